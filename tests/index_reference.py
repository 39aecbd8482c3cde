"""The batch index (eagcn_amd/csrc/index.hip) restated in plain numpy, device-free.

Everything the index holds is an integer function of the 0/1 adjacency and the one-hot relation tensors, so every comparison
made with this module is equality.  The word layout of the index buffers comes from eagcn_amd._lib (index_layout,
set_bond_lists); nothing here restates a byte offset.

    reference_index(adj, rels, ...)                -> dict of arrays, from the dense tensors
    reference_index_from_bonds(B, N, channels, ...) -> the same dict, from a bond list
    read_index(idx)                                -> the same dict, read back from an ops.BatchIndex / graph.StaticIndex
    compare_index(got, want)                       -> asserts equality field by field

What is NOT defined, and therefore never compared:
  * code rows of atoms without a bond (the dense scan leaves them as they were: no consumer gives such a row weight);
  * code columns at or beyond ceil(Nin/16)*16 when the caller's padded size Nin is below the capacity (no consumer reads a
    column beyond the 16-column tile of the molecule's last atom, and nat <= Nin);
  * list entries outside the listed ranges: a directed bond into an atom at or beyond nat counts in ecnt and edge0 but is
    listed nowhere, so a molecule's lists may be shorter than edge0[b+1] - edge0[b];
  * rows, tiles and blocks at or beyond meta[T], meta[NTILES], meta[NBLK].
"""
import ctypes as C

import numpy as np

from eagcn_amd import _lib as L


def _ceil16(n):
    return (int(n) + 15) // 16 * 16


def pack_blocks(nat, edge0, rb=256, maxm=16):
    """Row blocks: whole molecules, greedy in batch order.  A molecule joins the open block iff rows-so-far + nat <= rb and
    molecules-so-far + 1 <= maxm; an empty block takes its first molecule whatever its size; molecules without atoms count
    as molecules.  Returns blk [2*nblk, 4]: (first molecule, molecules, first packed row, rows), (first list entry, list
    entries, 0, 0)."""
    nat = [int(n) for n in nat]
    row0 = np.concatenate(([0], np.cumsum(nat))).astype(np.int64)
    groups, open_ = [], None
    for b, n in enumerate(nat):
        if open_ is not None and open_[2] + n <= rb and open_[1] + 1 <= maxm:
            open_[1] += 1
            open_[2] += n
        else:
            if open_ is not None:
                groups.append(open_)
            open_ = [b, 1, n]
    if open_ is not None:
        groups.append(open_)
    blk = np.zeros((2 * len(groups), 4), dtype=np.int32)
    for q, (first, cnt, rows) in enumerate(groups):
        blk[2 * q] = (first, cnt, row0[first], rows)
        blk[2 * q + 1] = (edge0[first], edge0[first + cnt] - edge0[first], 0, 0)
    return blk


def _finish(nz, code, N_cap, bad_adj, bad_rel, rb, maxm):
    """The index from the bond positions nz [B,Nin,Nin] (bool) and the per-view codes code [K,B,Nin,Nin] (uint8, 0 off the bonds)."""
    B, Nin, _ = nz.shape
    K = code.shape[0]
    N_cap = Nin if N_cap is None else int(N_cap)
    assert N_cap >= Nin
    ldc = _ceil16(N_cap)
    out = {'B': B, 'N': N_cap, 'Nin': Nin, 'K': K, 'ldc': ldc}
    deg = np.zeros((B, N_cap), dtype=np.int32)
    deg[:, :Nin] = nz.sum(axis=2)
    out['deg_bn'] = deg
    out['bonded'] = deg > 0
    idx = np.arange(1, N_cap + 1)
    nat = np.where(deg > 0, idx[None, :], 0).max(axis=1).astype(np.int32)
    ecnt = deg.sum(axis=1).astype(np.int32)
    tiles = (nat + 15) // 16
    out['nat'], out['ecnt'] = nat, ecnt
    for name, v in (('row0', nat), ('tile0', tiles), ('edge0', ecnt)):
        out[name] = np.concatenate(([0], np.cumsum(v.astype(np.int64)))).astype(np.int32)
    row0, edge0 = out['row0'], out['edge0']
    T, NT = int(row0[B]), int(out['tile0'][B])
    full = np.zeros((K, B, N_cap, ldc), dtype=np.uint8)
    full[:, :, :Nin, :Nin] = code
    out['code'] = full
    out['code_cols'] = _ceil16(Nin)
    # ---- packed rows and tiles
    row_mol = np.repeat(np.arange(B, dtype=np.int32), nat)
    row_loc = (np.arange(T, dtype=np.int32) - row0[row_mol]) if T else np.zeros(0, np.int32)
    out['row_mol'], out['row_loc'] = row_mol, row_loc.astype(np.int32)
    out['row_deg'] = deg[row_mol, row_loc].astype(np.int32)
    out['row_m'] = (out['row_deg'] > 0).astype(np.float32)
    out['row_info'] = np.stack([row_mol, row_loc, nat[row_mol], row0[row_mol]], axis=1).astype(np.int32).reshape(T, 4)
    tile_mol = np.repeat(np.arange(B, dtype=np.int32), tiles)
    tile_loc = (np.arange(NT, dtype=np.int32) - out['tile0'][tile_mol]) if NT else np.zeros(0, np.int32)
    out['tile_mol'] = tile_mol
    out['tile_info'] = np.stack([tile_mol, tile_loc, nat[tile_mol], row0[tile_mol]], axis=1).astype(np.int32).reshape(NT, 4)
    out['mol_info'] = np.stack([nat, row0[:B], edge0[:B], ecnt], axis=1).astype(np.int32)
    # ---- bond lists: bond (i, j) of molecule b is listed iff both ends are below nat[b]
    bb, ii, jj = np.where(nz)
    keep = (ii < nat[bb]) & (jj < nat[bb])
    bb, ii, jj = bb[keep], ii[keep], jj[keep]
    c64 = np.zeros(len(bb), dtype=np.uint64)
    for k in range(K):
        c64 |= code[k, bb, ii, jj].astype(np.uint64) << np.uint64(8 * k)
    NE = int(edge0[B])
    for fam, (major, minor) in (('row', (ii, jj)), ('col', (jj, ii))):
        order = np.lexsort((minor, major, bb))                        # molecule, then the list's atom, then the neighbour ascending
        b_s, a_s, n_s, c_s = bb[order], major[order], minor[order], c64[order]
        cnt = np.zeros(T, dtype=np.int64)
        np.add.at(cnt, row0[b_s] + a_s, 1)
        first = np.zeros(T, dtype=np.int64)
        for b in range(B):
            r0, n = int(row0[b]), int(nat[b])
            first[r0:r0 + n] = edge0[b] + np.concatenate(([0], np.cumsum(cnt[r0:r0 + n])[:-1])) if n else 0
        ptr = np.stack([first, cnt], axis=1).astype(np.int32).reshape(T, 2)
        nbr = np.full(NE, -1, dtype=np.int32)
        cod = np.zeros(NE, dtype=np.uint64)
        listed = np.zeros(NE, dtype=bool)
        if len(b_s):
            r = row0[b_s] + a_s
            start = np.concatenate(([True], r[1:] != r[:-1]))
            run0 = np.maximum.accumulate(np.where(start, np.arange(len(r)), 0))
            pos = first[r] + (np.arange(len(r)) - run0)
            nbr[pos], cod[pos], listed[pos] = n_s, c_s, True
        if fam == 'row':
            out['row_ptr'], out['nbr'], out['ecode'], out['listed'] = ptr, nbr, cod, listed
        else:
            out['col_ptr'], out['tnbr'], out['tcode'], out['tlisted'] = ptr, nbr, cod, listed
    # ---- row blocks
    out['blk'] = pack_blocks(nat, edge0, rb, maxm) if T > 0 else np.zeros((0, 4), dtype=np.int32)
    meta = np.zeros(L.META_WORDS, dtype=np.int32)
    meta[L.META_T], meta[L.META_NTILES], meta[L.META_NMAX], meta[L.META_NEDGE] = T, NT, int(nat.max()) if B else 0, NE
    meta[L.META_NLOG] = Nin if Nin < N_cap else 0
    meta[L.META_BAD_ADJ], meta[L.META_BAD_REL] = bad_adj, bad_rel
    meta[L.META_NBLK] = len(out['blk']) // 2
    out['meta'] = meta
    return out


def reference_index(adj, rels, N_cap=None, rb=256, maxm=16):
    """The index of the dense batch adj [B,Nin,Nin], rels[k] [B,C_k,Nin,Nin] (numpy) at capacity N_cap >= Nin."""
    adj = np.asarray(adj)
    nz = adj != 0                                              # (a NaN is a bond, and a bad one)
    bad_adj = int((nz & (adj != 1)).sum())
    code = np.zeros((len(rels),) + adj.shape, dtype=np.uint8)
    bad_rel = 0
    for k, r in enumerate(rels):
        r = np.asarray(r)
        one = r == 1
        ones = one.sum(axis=1)
        other = ((r != 0) & ~one).sum(axis=1)
        bad_rel += int((nz & ((ones != 1) | (other != 0))).sum())
        code[k] = np.where(nz, one.argmax(axis=1) + 1, 0).astype(np.uint8)
    return _finish(nz, code, N_cap, bad_adj, bad_rel, rb, maxm)


def reference_index_from_bonds(B, Nin, channels, bond_mol, bond_i, bond_j, bond_code, N_cap=None, rb=256, maxm=16):
    """The same dict from a bond list: bond_code [E,K], type per view.  BAD_ADJ counts bonds out of range or listed again,
    BAD_REL bonds with a type beyond its view's channels (both as eagcn_index_from_bonds reports them)."""
    bm, bi, bj = (np.asarray(a, dtype=np.int64) for a in (bond_mol, bond_i, bond_j))
    bc = np.asarray(bond_code).reshape(len(bm), len(channels)).astype(np.int64)
    ok = (bm >= 0) & (bm < B) & (bi >= 0) & (bi < Nin) & (bj >= 0) & (bj < Nin)
    bad_adj = int((~ok).sum())
    bm, bi, bj, bc = bm[ok], bi[ok], bj[ok], bc[ok]
    _, firsts = np.unique(np.stack([bm, bi, bj], axis=1), axis=0, return_index=True) if len(bm) else (None, np.zeros(0, np.int64))
    bad_adj += len(bm) - len(firsts)
    firsts = np.sort(firsts)
    bm, bi, bj, bc = bm[firsts], bi[firsts], bj[firsts], bc[firsts]
    bad_rel = int((bc >= np.asarray(channels)[None, :]).any(axis=1).sum())
    nz = np.zeros((B, Nin, Nin), dtype=bool)
    nz[bm, bi, bj] = True
    code = np.zeros((len(channels), B, Nin, Nin), dtype=np.uint8)
    for k in range(len(channels)):
        code[k, bm, bi, bj] = (bc[:, k] + 1).astype(np.uint8)
    return _finish(nz, code, N_cap, bad_adj, bad_rel, rb, maxm)


def densify(B, N, channels, bond_mol, bond_i, bond_j, bond_code):
    """(adj [B,N,N], [rel_k [B,C_k,N,N]]) float32 of a bond list, as the reference's collate pads them."""
    adj = np.zeros((B, N, N), dtype=np.float32)
    adj[bond_mol, bond_i, bond_j] = 1.0
    rels = []
    for k, c in enumerate(channels):
        r = np.zeros((B, c, N, N), dtype=np.float32)
        r[bond_mol, np.asarray(bond_code)[:, k], bond_i, bond_j] = 1.0
        rels.append(r)
    return adj, rels


def read_index(idx):
    """An ops.BatchIndex or graph.StaticIndex as the dict reference_index returns (numpy, trimmed to the extents in meta).
    The bond-list arrays are found from the Batch struct's own pointers relative to the tensors that hold them."""
    c = idx.c
    B, N, K, ldc = int(c.B), int(c.N), int(c.K), int(c.ldc)
    blob_lay, rows_lay = L.index_layout(B, N, int(c.T), int(c.n_tiles))
    blob = idx._blob.cpu().numpy()
    rows = idx._rows.cpu().numpy()
    out = {'B': B, 'N': N, 'K': K, 'ldc': ldc}
    for name in ('deg_bn', 'nat', 'row0', 'tile0', 'meta', 'ecnt', 'edge0'):
        assert getattr(c, name) == idx._blob.data_ptr() + 4 * blob_lay[name].start, name
        out[name] = blob[blob_lay[name]].copy()
    out['deg_bn'] = out['deg_bn'].reshape(B, N)
    out['bonded'] = out['deg_bn'] > 0
    meta = out['meta']
    T, NT, NE = int(meta[L.META_T]), int(meta[L.META_NTILES]), int(meta[L.META_NEDGE])
    assert T <= c.T and NT <= c.n_tiles
    out['code'] = idx.code.cpu().numpy().reshape(K, B, N, ldc)
    for name in ('row_info', 'tile_info', 'row_mol', 'row_loc', 'row_deg', 'row_m', 'tile_mol'):
        assert getattr(c, name) == idx._rows.data_ptr() + 4 * rows_lay[name].start, name
        out[name] = rows[rows_lay[name]].copy()
    out['row_m'] = out['row_m'].view(np.float32)[:T]
    out['row_info'] = out['row_info'].reshape(-1, 4)[:T]
    out['tile_info'] = out['tile_info'].reshape(-1, 4)[:NT]
    for name in ('row_mol', 'row_loc', 'row_deg'):
        out[name] = out[name][:T]
    out['tile_mol'] = out['tile_mol'][:NT]
    ptrs = idx._ptrs.cpu().numpy()
    edges = idx._edges.cpu().numpy()

    def words(t, host, field, n):
        off = getattr(c, field) - t.data_ptr()
        assert off >= 0 and off % 4 == 0 and off // 4 + n <= host.size, (field, off, n, host.size)
        return host[off // 4: off // 4 + n].copy()
    out['row_ptr'] = words(idx._ptrs, ptrs, 'row_ptr', 2 * T).reshape(T, 2)
    out['col_ptr'] = words(idx._ptrs, ptrs, 'col_ptr', 2 * T).reshape(T, 2)
    out['mol_info'] = words(idx._ptrs, ptrs, 'mol_info', 4 * B).reshape(B, 4)
    nblk = int(meta[L.META_NBLK])
    out['blk'] = words(idx._ptrs, ptrs, 'blk', 8 * nblk).reshape(2 * nblk, 4) if c.blk else None
    NE = min(NE, int(c.E))
    out['nbr'] = words(idx._edges, edges, 'nbr', NE)
    out['tnbr'] = words(idx._edges, edges, 'tnbr', NE)
    out['ecode'] = words(idx._edges, edges, 'ecode', 2 * NE).view(np.uint64)
    out['tcode'] = words(idx._edges, edges, 'tcode', 2 * NE).view(np.uint64)
    return out


def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def compare_index(got, want, lists=True, blocks=True):
    """got == want on every defined field; the failure names the first differing field, molecule and row."""
    for name in ('B', 'N', 'K', 'ldc'):
        assert got[name] == want[name], (name, got[name], want[name])
    B = want['B']
    row0 = want['row0']

    def where(r):                                                  # packed row -> 'molecule b row i'
        b = int(np.searchsorted(row0, r, side='right') - 1)
        return 'molecule %d row %d' % (b, r - int(row0[b]))
    for name in ('deg_bn', 'nat', 'ecnt', 'row0', 'tile0', 'edge0'):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = _first(g != w)
            raise AssertionError('%s differs at %s (molecule %d): got %d, want %d' % (name, at, at[0], g[at], w[at]))
    skip = (L.META_NBLK,) if not blocks else ()
    for word in (L.META_T, L.META_NMAX, L.META_NTILES, L.META_BAD_ADJ, L.META_BAD_REL, L.META_NEDGE, L.META_OVERFLOW,
                 L.META_EDGE_OVERFLOW, L.META_NLOG, L.META_NBLK):
        if word not in skip:
            assert int(got['meta'][word]) == int(want['meta'][word]), ('meta[%d]' % word, int(got['meta'][word]), int(want['meta'][word]))
    cols = want.get('code_cols', want['ldc'])
    m = want['bonded'][None, :, :, None]
    g, w = got['code'][..., :cols] * m, want['code'][..., :cols] * m
    if not np.array_equal(g, w):
        k, b, i, j = _first(g != w)
        raise AssertionError('code differs at view %d molecule %d row %d column %d: got %d, want %d' % (k, b, i, j, g[k, b, i, j], w[k, b, i, j]))
    for name in ('row_mol', 'row_loc', 'row_deg', 'row_m', 'row_info', 'tile_mol', 'tile_info', 'mol_info'):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = _first(g != w)
            what = where(at[0]) if name.startswith('row') else ('molecule %d' % at[0] if name == 'mol_info' else 'tile %d' % at[0])
            raise AssertionError('%s differs at %s (%s): got %s, want %s' % (name, at, what, g[at], w[at]))
    if lists:
        for ptr, nbr, cod, lst in (('row_ptr', 'nbr', 'ecode', 'listed'), ('col_ptr', 'tnbr', 'tcode', 'tlisted')):
            g, w = got[ptr], want[ptr]
            assert g.shape == w.shape, (ptr, g.shape, w.shape)
            if not np.array_equal(g, w):
                at = _first(g != w)
                raise AssertionError('%s differs at %s: got %s, want %s' % (ptr, where(at[0]), g[at[0]], w[at[0]]))
            mask = want[lst]
            for name in (nbr, cod):
                g, w = got[name], want[name]
                assert len(g) == len(w), (name, len(g), len(w))
                bad = mask & (g != w)
                if bad.any():
                    e = _first(bad)[0]
                    r = int(np.searchsorted(want[ptr][:, 0] + want[ptr][:, 1], e, side='right'))
                    raise AssertionError('%s differs at entry %d (%s): got %d, want %d' % (name, e, where(r), g[e], w[e]))
    if blocks and got.get('blk') is not None:
        g, w = got['blk'], want['blk']
        assert g.shape == w.shape, ('blk', g.shape, w.shape)
        if not np.array_equal(g, w):
            q = _first(g != w)[0]
            raise AssertionError('blk differs at record %d (block %d, first molecule %d): got %s, want %s'
                                 % (q, q // 2, int(w[q & ~1][0]), g[q], w[q]))
