"""The case table of the matrix-core aggregation's dispatch space (csrc/agg.hip), shared by tests/test_gpu_agg_dispatch.py (which
runs the cases against the float64 oracle), its subprocess body tests/agg_dispatch_check.py and tests/test_agg_dispatch_cpu.py
(which asserts that the table reaches every kernel form and that every batch is valid input).

Two things live here, both device-free:
  * the batches (numpy, deterministic) and the cases (structure, widths, switch of the work distribution);
  * `dispatch(...)`: what a launch of the dense aggregation takes for a batch and a layer, RESTATED from the description of the
    policy ("the dispatch space of the matrix-core aggregation"), never by calling the library:
        tmax   = the widest view's count of 16-column tiles;  nchunk = ceil(tmax / 9);  CT = ceil(tmax / nchunk), and CT = 8 runs
                 the 9-tile instantiation with its last tile masked off;
        chunk cc of view k starts at tile ct0 = cc * CT: the workgroup returns when ct0 >= tiles of view k, else it runs
                 nct = min(CT, tiles of view k - ct0) tiles;
        B <= EAGCN_AGG_KSPLIT_MAXB (256): one workgroup per row tile, K split over its waves, at most 1024 workgroups along x;
        else one wave per row tile, four per workgroup, at most 512 workgroups (2048 tiles) along x;  beyond a cap the kernel loops;
        the wave form hands its tiles out XCD-contiguously when tiles >= 4 B (the live workgroups of a pass are remapped by a
                 bijection with a remainder branch for a count that is no multiple of 8);
        the edge gradients: one workgroup per 16 packed rows, at most 1024;  in the wave form their row blocks are handed out
                 XCD-contiguously when rows >= 64 B;  the histogram leaves atomically (one-hot relations) or as one slab per
                 workgroup (code-book relations);  a row's hit queue (64 slots) is flushed early once it holds more than 48 hits
                 (the diagonal is queued with the bonds);  a second 256-column segment of the code row is walked when the
                 molecule has more than 256 atoms.
"""
import functools

import numpy as np

from eagcn_amd.synthetic import MolBatch, make_batch

MAX_CT = 9                      # column tiles per workgroup (EAGCN_AGG_MAXCT is a debug switch and stays at its default)
KSPLIT_MAXB = 256               # EAGCN_AGG_KSPLIT_MAXB by default
KSPLIT_CAP, WAVE_CAP, EDGE_CAP = 1024, 512, 1024
HIT_FLUSH = 48                  # queued hits beyond which a row's queue is flushed before the code row is finished


def cdiv(a, b):
    return -(-int(a) // int(b))


def pad16(w):
    return (int(w) + 15) // 16 * 16


# ---- batches -----------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = (1, 15, 16, 17, 31, 33, 47, 2, 9, 24, 40, 5)
BIG_SIZES = (300, 257, 40, 17, 2)
GENERAL_CHANNELS = (6, 4, 3, 2, 2)


def _add_bonds(mb, b, pairs, rng):
    """Undirected bonds `pairs` of molecule b (a pair (i, i) is a self bond, listed once), one random type per view."""
    e, c = [], []
    for i, j in pairs:
        code = [int(rng.integers(0, ch)) for ch in mb.rel_channels]
        for a, d in ((i, j),) if i == j else ((i, j), (j, i)):
            e.append((b, a, d))
            c.append(code)
    mb.edges = np.concatenate([mb.edges, np.asarray(e, dtype=np.int64).reshape(-1, 3)])
    mb.codes = np.concatenate([mb.codes, np.asarray(c, dtype=np.int64).reshape(-1, mb.codes.shape[1])])


def _degrees(mb):
    deg = np.zeros((mb.B, mb.N), dtype=np.int64)
    np.add.at(deg, (mb.edges[:, 0], mb.edges[:, 1]), 1)
    return deg


@functools.lru_cache(maxsize=None)
def batch(kind, *args):
    """The batch of a case: a MolBatch (and, for 'general', its relation palettes: see general_dense)."""
    if kind == 'ragged':                       # 12 molecules, 1..47 atoms, isolated atoms, one self bond
        channels, = args
        mb = make_batch(B=len(RAGGED_SIZES), n_max=max(RAGGED_SIZES), sizes=np.asarray(RAGGED_SIZES), rel_channels=channels, seed=11,
                        isolated_frac=0.08, n_tasks=3)
        i = int(_degrees(mb)[6].argmax())
        _add_bonds(mb, 6, [(i, i)], np.random.default_rng(5))
        return mb
    if kind == 'uniform':                      # B molecules of exactly n atoms; view 0: every bond of molecule b has type b mod 12
        B, n = args
        mb = make_batch(B=B, n_max=n, all_full=True, rel_channels=(12, 2), seed=100 + B, n_tasks=3)
        mb.codes[:, 0] = mb.edges[:, 0] % 12
        return mb
    if kind == 'big':                          # padded beyond 256 atoms; a hub atom with 60 more bonds, some to atoms >= 256
        channels, = args
        mb = make_batch(B=len(BIG_SIZES), n_max=max(BIG_SIZES), sizes=np.asarray(BIG_SIZES), rel_channels=channels, seed=23, n_tasks=3)
        rng = np.random.default_rng(7)
        hub = 5
        have = {int(j) for b, i, j in mb.edges if b == 0 and i == hub}
        low = [j for j in range(20, 256, 7) if j not in have and j != hub][:30]
        high = [j for j in range(256, 300) if j not in have][:30]
        _add_bonds(mb, 0, [(hub, j) for j in low + high], rng)
        i = int(_degrees(mb)[1].argmax())
        _add_bonds(mb, 1, [(i, i)], rng)
        return mb
    if kind == 'general':                      # code-book relations: N = 21, real-valued channel vectors from small palettes
        B, = args
        return make_batch(B=B, n_max=21, n_med=9, rel_channels=tuple(5 + k for k in range(len(GENERAL_CHANNELS))), seed=17 + B,
                          n_tasks=2, task='reg', isolated_frac=0.1)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def general_palettes(B):
    """Per view, the real-valued channel vectors a bond's relation entry is drawn from ([5 + k, C_k]; multi-hot, fractional)."""
    rng = np.random.default_rng(1000 + B)
    return tuple(np.round(rng.normal(0.0, 1.0, size=(5 + k, c)), 2).astype(np.float32) * (rng.random((5 + k, c)) < 0.6)
                 for k, c in enumerate(GENERAL_CHANNELS))


def general_dense(B):
    """(adj, afm, rel_1..rel_5, size) of the code-book batch as numpy arrays -- what the reference's collate would deliver --
    and the per-molecule tuples eagcn_amd.collate.collate_compact takes."""
    mb, pal = batch('general', B), general_palettes(B)
    e = mb.edges
    adj = np.zeros((B, mb.N, mb.N), dtype=np.float32)
    adj[e[:, 0], e[:, 1], e[:, 2]] = 1.0
    rels = []
    for k, p in enumerate(pal):
        r = np.zeros((B, p.shape[1], mb.N, mb.N), dtype=np.float32)
        r[e[:, 0], :, e[:, 1], e[:, 2]] = p[mb.codes[:, k]]
        rels.append(r)
    mols = []
    for b in range(B):
        n = int(mb.sizes[b])
        mols.append((adj[b, :n, :n].copy(), mb.afm[b, :n].copy()) + tuple(r[b, :, :n, :n].copy() for r in rels) +
                    (mb.labels[b].copy(), 'm%d' % b, None, b))
    return [adj, mb.afm] + rels + [mb.sizes], mols


def shape(mb):
    """(B, N, nat per molecule, packed rows T, row tiles, largest number of queued hits of a row) of a batch, as the index
    defines them: nat = 1 + the last atom that has a bond."""
    deg = _degrees(mb)
    idx = np.arange(1, mb.N + 1)
    nat = np.where(deg > 0, idx[None, :], 0).max(axis=1)
    diag = np.zeros_like(deg)
    loops = mb.edges[mb.edges[:, 1] == mb.edges[:, 2]]
    np.add.at(diag, (loops[:, 0], loops[:, 1]), 1)
    hits = int((deg + 1 - diag).max()) if deg.size else 0      # a row's bonds plus its diagonal (queued once, bond or not)
    return dict(B=mb.B, N=mb.N, nat=nat, T=int(nat.sum()), tiles=int(((nat + 15) // 16).sum()), hits=hits)


# ---- the restated dispatch -----------------------------------------------------------------------------------------------------
def view_widths(structure, widths):
    """The per-view widths of a layer: Weighted_sum gives every view the sum (reference models.py:33-47)."""
    return [sum(widths)] * len(widths) if structure == 'Weighted_sum' else list(widths)


def remap(n, bx):
    """The XCD-contiguous hand-out of n live workgroups: workgroup bx (on XCD bx mod 8) -> position."""
    q8, r8, x = n >> 3, n & 7, bx & 7
    return x * q8 + min(x, r8) + (bx >> 3)


def dispatch(widths, B, T, tiles, nat_max, hits, maxb=None, general=False):
    """What the dense aggregation of a layer with per-view `widths` takes on a batch of B molecules, T packed rows and `tiles`
    row tiles (see the module docstring)."""
    maxb = KSPLIT_MAXB if maxb is None else maxb
    vt = [pad16(w) // 16 for w in widths]
    tmax = max(vt)
    nchunk = cdiv(tmax, MAX_CT)
    ct = cdiv(tmax, nchunk)
    d = dict(tmax=tmax, nchunk=nchunk, masked=ct == 8, CT=9 if ct == 8 else ct)
    ct = d['CT']
    d['nct'] = sorted({min(ct, t - cc * ct) for t in vt for cc in range(nchunk) if cc * ct < t})
    d['skipped'] = any(cc * ct >= t for t in vt for cc in range(nchunk))
    # nct < CT for some view and chunk (the masked tile of an 8-tile layer is not meant: that is `masked`)
    d['partial'] = any(n < ct for n in d['nct']) and not (d['masked'] and d['nct'] == [8])
    d['form'] = 'ksplit' if B <= maxb else 'wave'
    wave = d['form'] == 'wave'
    gx = max(1, min(cdiv(tiles, 4), WAVE_CAP)) if wave else max(1, min(tiles, KSPLIT_CAP))
    per_pass = gx * 4 if wave else gx
    d['agg_wg'], d['agg_passes'] = gx, cdiv(tiles, per_pass)
    d['tile_handout'] = wave and tiles >= 4 * B
    # live workgroups of every pass (the remainder branch of the bijection is taken when the count is no multiple of 8)
    d['tile_live'] = [min(gx, cdiv(tiles - p * per_pass, 4)) for p in range(d['agg_passes'])] if wave else []
    d['tile_rem'] = [n & 7 for n in d['tile_live']] if d['tile_handout'] else []
    blocks = cdiv(T, 16)
    egx = max(1, min(blocks, EDGE_CAP))
    d['edge_wg'], d['edge_passes'] = egx, cdiv(blocks, egx)
    d['edge_handout'] = wave and T >= 64 * B
    d['edge_rem'] = (egx & 7) if d['edge_handout'] else None
    d['edge_out'] = 'slab' if general else 'atomic'
    d['flush'] = hits > HIT_FLUSH
    d['segments'] = cdiv(max(nat_max, 1), 256)
    return d


def describe(d):
    """The dispatch of one layer in the words the result lines carry."""
    s = 'CT%d%s x%d %s pass %d' % (d['CT'], 'm' if d['masked'] else '', d['nchunk'], d['form'], d['agg_passes'])
    if d['tile_handout']:
        s += ' xcd(rem %s)' % '/'.join(str(r) for r in d['tile_rem'])
    s += ' | edge %s pass %d' % (d['edge_out'], d['edge_passes'])
    if d['edge_handout']:
        s += ' xcd(rem %d)' % d['edge_rem']
    if d['flush']:
        s += ' flush'
    if d['segments'] > 1:
        s += ' seg %d' % d['segments']
    return s


# ---- the cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """One model on one batch.  child: the subprocess the case shares with others (None: runs in the pytest process);
    maxb: EAGCN_AGG_KSPLIT_MAXB of that child (None: the default);  n_atoms: the largest molecule the case states;
    edge_ref: how att.weight / self_r are held where the rule does not apply to them (None: no exception; 'lds': against a run of
    the bond-list path; 'sentinel': no entry off by more than 1 % of its own value)."""

    def __init__(self, name, child, maxb, structure, channels, w1, w2, batch_key, n_atoms, edge_ref=None, general=False, typed=False):
        self.name, self.child, self.maxb, self.structure, self.channels = name, child, maxb, structure, tuple(channels)
        self.w1, self.w2, self.batch_key, self.n_atoms, self.edge_ref, self.general = list(w1), list(w2), batch_key, n_atoms, edge_ref, general
        self.typed = typed                       # view 0 carries the bond type 1 + (b mod 12) on every bond of molecule b

    def batch(self):
        return batch(*self.batch_key)

    def layers(self):
        """The restated dispatch of the two layers."""
        s = shape(self.batch())
        return [dispatch(view_widths(self.structure, w), s['B'], s['T'], s['tiles'], int(s['nat'].max()), s['hits'], self.maxb, self.general)
                for w in (self.w1, self.w2)]

    def line(self):
        return ' || '.join(describe(d) for d in self.layers())


CH3 = (6, 3, 2)
# (a) the CT sweep: equal widths with tmax = 1..10, 16, 19 over the two layers, a width that is no multiple of 16 (100: 7 tiles),
# unequal views ([160, 48, 16]: view 2 and 3 end before ct0 of the second chunk; [112, 40, 16]: nct < CT in the first chunk)
_EQUAL = [(16, 32), (48, 64), (80, 96), (112, 128), (144, 160), (256, 304), (100, 100)]
_GROUPS = (0, 0, 1, 1, 2, 2, 0)                   # the child a width pair goes to (the wide pair alone with the narrow ones)


def _ct_sweep():
    out = []
    for form, maxb in (('ksplit', None), ('wave', 0)):
        for (a, b), g in zip(_EQUAL, _GROUPS):
            out.append(Case('ct-%s-concate-%d-%d' % (form, a, b), 'ct-%s-%d' % (form, g), maxb, 'Concate', CH3, [a] * 3, [b] * 3,
                            ('ragged', CH3), 47))
            # (Weighted_sum gives every view the SUM of the widths it is built with)
            out.append(Case('ct-%s-weighted-%d-%d' % (form, a, b), 'ct-%s-%d' % (form, g), maxb, 'Weighted_sum', CH3, [a, 0, 0], [b, 0, 0],
                            ('ragged', CH3), 47))
        out.append(Case('ct-%s-concate-unequal' % form, 'ct-%s-1' % form, maxb, 'Concate', CH3, [160, 48, 16], [112, 40, 16],
                        ('ragged', CH3), 47))
    return out


CH2 = (12, 2)
# (b) grid caps and XCD hand-outs
_CAPS = [
    # K-split forced at 600 molecules: 1800 tiles > 1024, a second pass
    Case('caps-ksplit-600x33', 'caps-ksplit', 100000, 'Concate', CH2, [16, 16], [32, 16], ('uniform', 600, 33), 33, typed=True),
    # wave form: 3300 tiles > 2048 and 36300 rows > 16384: a second pass in both halves of the co-launch, no hand-out
    Case('caps-wave-1100x33', 'caps-wave-1100', None, 'Concate', CH2, [16, 16], [32, 16], ('uniform', 1100, 33), 33, typed=True),
    # tiles >= 4 B: tile hand-out with 375 live workgroups (remainder 7);  rows >= 64 B and > 16384: edge hand-out at the cap
    Case('caps-wave-300x70', 'caps-wave-300', None, 'Concate', CH2, [16, 16], [32, 16], ('uniform', 300, 70), 70, edge_ref='lds', typed=True),
    # edge hand-out with a workgroup count that is no multiple of 8 (569), CT = 5
    Case('caps-wave-130x70', 'caps-wave-130', 0, 'Concate', CH2, [80, 80], [16, 32], ('uniform', 130, 70), 70, edge_ref='lds', typed=True),
]
# (c) the default policy, in the pytest process, no switch set
_POLICY = [Case('policy-big-%s' % s.lower(), None, None, s, CH3, w1, w2, ('big', CH3), 300, edge_ref='sentinel')
           for s, w1, w2 in (('Concate', [128] * 3, [208] * 3), ('Weighted_sum', [128, 0, 0], [208, 0, 0]))]
_POLICY += [Case('policy-codebook-%d' % B, None, None, 'Concate', GENERAL_CHANNELS, [96, 40, 128, 16, 16], [112] * 5, ('general', B), 21,
                 general=True) for B in (260, 24)]

CASES = _ct_sweep() + _CAPS + _POLICY
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def children():
    """{child: [case names]} of the cases that run in subprocesses, in table order."""
    out = {}
    for c in CASES:
        if c.child is not None:
            out.setdefault(c.child, []).append(c.name)
    return out


def child_env(child):
    """The switches of a child: every child forces the dense aggregation; one work-distribution threshold per child."""
    maxbs = {BY_NAME[n].maxb for n in children()[child]}
    assert len(maxbs) == 1, (child, maxbs)
    env = {'EAGCN_AGG': 'dense'}
    maxb, = maxbs
    if maxb is not None:
        env['EAGCN_AGG_KSPLIT_MAXB'] = str(maxb)
    return env
