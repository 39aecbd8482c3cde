"""The device-side atom-representation dump (eagcn_amd.analysis.RepBuffers / dump_atom_rep over csrc/reps.hip: eagcn_rep_gather)
against ``atom_rep.cpu()`` indexed by the sub-type mask -- bit for bit, in the order of the reference's loop over the flattened batch
(train.py:264-268) -- and the small pieces around it (as_reference, confusion_matrix, the model-to-clusters path)."""
import copy

import numpy as np
import pytest
import torch

from eagcn_amd import EAGCN
from eagcn_amd.analysis import RepBuffers, confusion_matrix, dump_atom_rep, kmeans
from eagcn_amd.models import LazyAtomRep
from eagcn_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu

CH = (28, 4, 2, 2, 2)
KW = {'Concate': dict(widths1=[8, 6, 10, 7, 5], widths2=[12, 10, 7, 9, 5]), 'Weighted_sum': dict(widths1=[10] * 5, widths2=[13] * 5)}


def _model(structure, graph=False, **extra):
    torch.manual_seed(4)
    m = EAGCN(28, 24, n_den1=16, n_den2=8, nclass=2, dropout=0.0, structure=structure, n_layers=2, graph=graph, **KW[structure], **extra)
    return m.cuda().eval()


def _batch(seed, n_max=20, B=5):
    mb = make_batch(B=B, n_max=n_max, n_med=7, rel_channels=CH, seed=seed, isolated_frac=0.25, n_tasks=2)
    rs = np.random.RandomState(seed)
    subtype = torch.from_numpy(rs.randint(0, 21, size=(B, mb.N)))          # 0, 19, 20 are not selected; atoms beyond nat[b] may be
    index = torch.arange(B, dtype=torch.int64) + 100 * seed
    return mb, subtype, index


def _expected(dense, subtype, index, lo=1, hi=18):
    B, N, F = dense.shape
    mask = ((subtype >= lo) & (subtype <= hi)).view(-1)
    return dense.reshape(-1, F)[mask], subtype.view(-1)[mask].to(torch.int32), index.view(B, 1).expand(B, N).reshape(-1)[mask]


def _two_appends(model, n_max=(20, 17), cap=120):
    buf = RepBuffers('cuda', cap=cap)
    want = []
    with torch.no_grad():                                                  # (a Concate forward skips the top layer's matrix: materializer)
        for j, nm in enumerate(n_max):
            mb, subtype, index = _batch(11 + j, nm)
            out, rep, grep = model(*[t.cuda() for t in mb.dense()])
            assert isinstance(rep, LazyAtomRep) and (rep._materialize is not None) == (model.structure == 'Concate')
            buf.append(rep, subtype, index, graph_rep=grep, labels=torch.from_numpy(mb.labels), outputs=out)
            dense = rep.cpu()                                              # (after the append: the packed path was taken)
            beyond = torch.arange(mb.N)[None, :] >= torch.from_numpy(mb.sizes)[:, None]
            assert dense.shape[:2] == (mb.B, mb.N) and (beyond & (subtype >= 1) & (subtype <= 18)).any()
            want.append(_expected(dense, subtype, index))
    d = buf.finish()
    X, sub, mol = (torch.cat([w[i] for w in want]) for i in range(3))
    assert d.X.shape == X.shape and X.shape[0] > 60
    assert torch.equal(d.X.cpu(), X)                                      # bit for bit, the second batch behind the device counter
    assert torch.equal(d.subtype.cpu(), sub) and torch.equal(d.mol_index.cpu(), mol)
    assert int(buf.count.item()) == X.shape[0]
    return buf, d


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_two_appends_equal_the_masked_dense_tensor(structure, graph):
    model = _model(structure, graph)
    buf, d = _two_appends(model)
    assert buf.cap >= buf.bound == 5 * 20 + 5 * 17 and buf.cap > 120      # grew once, the first batch's rows were carried over
    assert d.graph_rep.shape[0] == d.index.shape[0] == d.labels.shape[0] == d.outputs.shape[0] == 10


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_bucketed_batch_uses_the_batch_own_padding(structure):
    model = _model(structure, True, n_bucket=16)
    _two_appends(model, n_max=(19, 23))                                    # both in the bucket (16, 32]: N_in < N = 32
    assert len(model._runners) == 1


def test_dense_tensor_input_and_other_range():
    model = _model('Concate')
    mb, subtype, index = _batch(21)
    with torch.no_grad():
        _, rep, _ = model(*[t.cuda() for t in mb.dense()])
    dense = rep.cpu()
    buf = RepBuffers('cuda', subtype_range=(3, 9), cap=16)
    buf.append(dense.cuda(), subtype, index)
    buf.append(dense.cuda(), subtype.cuda(), index.cuda() + 7)
    d = buf.finish()
    X, sub, mol = _expected(dense, subtype, index, 3, 9)
    assert torch.equal(d.X.cpu(), torch.cat([X, X])) and torch.equal(d.subtype.cpu(), torch.cat([sub, sub]))
    assert torch.equal(d.mol_index.cpu(), torch.cat([mol, mol + 7]))
    assert d.graph_rep is None and d.labels is None and d.index.shape == (10,)
    empty = RepBuffers('cuda', subtype_range=(30, 40))
    empty.append(dense.cuda(), subtype, index)
    assert empty.finish().X.shape == (0, dense.shape[2])


def test_dump_atom_rep_restores_mode_keeps_statistics_and_has_the_reference_structure():
    model = _model('Concate').train()
    before = copy.deepcopy(model.state_dict())
    batches, want = [], []
    for j in range(3):
        mb, subtype, index = _batch(31 + j)
        labels = torch.from_numpy(mb.labels)
        if j == 1:
            batch = mb.compact('cuda')
        else:
            batch = tuple(t.cuda() for t in mb.dense())
        batches.append((batch, labels, subtype, index))
    buf = dump_atom_rep(model, batches)
    assert model.training
    after = model.state_dict()
    for name in before:
        assert torch.equal(before[name], after[name]), name
    model.eval()
    with torch.no_grad():
        for (batch, labels, subtype, index), j in zip(batches, range(3)):
            out, rep, grep = model.forward_compact(*batch) if j == 1 else model(*batch)
            want.append(_expected(rep.cpu(), subtype, index) + (grep.cpu(), out.cpu()))
    d = buf.finish()
    assert torch.equal(d.X.cpu(), torch.cat([w[0] for w in want]))
    assert torch.equal(d.subtype.cpu(), torch.cat([w[1] for w in want])) and torch.equal(d.mol_index.cpu(), torch.cat([w[2] for w in want]))
    assert torch.equal(d.graph_rep.cpu(), torch.cat([w[3] for w in want])) and torch.equal(d.outputs.cpu(), torch.cat([w[4] for w in want]))
    # train.py:272 / :280
    atoms, mols = buf.as_reference()
    n, F = d.X.shape
    assert len(atoms) == 3 and len(atoms[0]) == len(atoms[1]) == len(atoms[2]) == n
    assert atoms[0][5].shape == (F,) and atoms[0][5].dtype == np.float32 and np.array_equal(atoms[0][5], d.X[5].cpu().numpy())
    assert atoms[1][5].shape == () and int(atoms[1][5]) == int(d.subtype[5]) and 1 <= int(atoms[1][5]) <= 18
    assert atoms[2][5].shape == (1,) and int(atoms[2][5][0]) == int(d.mol_index[5])
    assert len(mols) == 4 and mols[0].shape == (15, d.graph_rep.shape[1]) and mols[1].shape == (15, 1)
    assert mols[2].shape == (15, 2) and mols[3].shape == (15, 2)
    assert np.array_equal(mols[1][:, 0], np.concatenate([np.arange(5) + 100 * (31 + j) for j in range(3)]))
    assert np.array_equal(np.asarray(atoms[0]), d.X.cpu().numpy())


def test_confusion_matrix_equals_sklearn():
    from sklearn.metrics import confusion_matrix as sk_cm
    rs = np.random.RandomState(2)
    y, c = rs.randint(0, 18, 4000), rs.randint(0, 6, 4000)
    got = confusion_matrix(torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda().to(torch.int32), 18, 6)
    want = sk_cm(y, c, labels=np.arange(18))[:, :6]
    assert got.is_cuda and got.shape == (18, 6) and np.array_equal(got.cpu().numpy(), want)


def test_model_to_clusters():
    model = _model('Concate', True)
    batches = []
    for j in range(4):
        mb, subtype, index = _batch(41 + j, B=8)
        batches.append((tuple(t.cuda() for t in mb.dense()), torch.from_numpy(mb.labels), subtype, index))
    buf = dump_atom_rep(model, batches, subtype_range=(3, 9))              # one element's sub-types
    d = buf.finish()
    n = d.X.shape[0]
    assert n > 60
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    res = kmeans(d.X, 6, generator=gen)
    assert res.labels.shape == (n,) and int(res.counts.sum()) == n and res.centers.shape == (6, d.X.shape[1])
    cm = confusion_matrix(d.subtype - 3, res.labels, 7, 6)
    assert int(cm.sum()) == n and torch.equal(cm.sum(0), res.counts)
