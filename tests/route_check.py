"""Run by test_host_cpu.py in a subprocess per environment (the library reads its switches once): eagcn_layer_route over a cross
product of batches, layers and calls against the routes WRITTEN OUT here from the policy's description (DESIGN.md "the route of
a layer call"), never derived from the library; the invariants of a route; that a call which sets the reserved field
eagcn_layer_bufs.aux_stream is refused; and, with no switch set, the pinned sizes of the three carvings.  No GPU: every address
is a made-up multiple of 4096 and nothing is dereferenced."""
import ctypes as C
import importlib.util
import itertools
import os

# the binding alone, by path: importing the package would pull torch into each of these short-lived processes
_spec = importlib.util.spec_from_file_location('eagcn_lib_binding', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 'eagcn_amd', '_lib.py'))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)

CONCATE, WEIGHTED = L.STRUCT_CONCATE, L.STRUCT_WEIGHTED
# out[] of eagcn_layer_route (include/eagcn_hip.h)
(FWD_PROD, FWD_SPLIT, FWD_AGG, BWD_AGG, BN2, ROWS_FIRST, ROWS_LATE, STORE_DH, EDGE, EDGE_ATOMIC, BWD_PROD, BWD_SPLIT, DEFER,
 PLANES_ONLY) = range(14)
FWD_PLANES, FWD_BALANCED, FWD_TILED, FWD_REFUSED = 1, 2, 3, 4
ELEMENTWISE, REDUCE_APPLY, STAGED_DH, STAGED_UPSTREAM, STAGED_ROWMASK = 1, 2, 3, 4, 5
WITH_LAGG, COLAUNCH = 1, 2
ERR_ARG = -1                                                     # EAGCN_ERR_ARG
PLANES_PAIR, PLANES_DW, PLANES_DX, G3_XK, G3_SCATTER, TILED_PAIR, TILED_SEPARATE, TILED_DX, BWD_REFUSED = range(1, 10)

_next = [1 << 24]


def fake():
    _next[0] += 1 << 20
    return _next[0]


# name -> (B, N, T, bond lists, code-book relation)
BATCHES = {'tox21': (256, 132, 4809, True, False), 'hiv': (1024, 222, 25000, True, False), 'no_lists': (256, 132, 4809, False, False),
           'n300': (64, 300, 6000, True, False), 'codebook': (256, 132, 4809, True, True), 'empty': (256, 132, 0, True, False),
           'n256': (64, 256, 8000, True, False)}
# name -> (input segments (width, pad), view width, x given, x_planes given, has_dx, has_drain_out)
LAYERS = {'first': ([(24, 24)], 80, True, False, 0, 0), 'hidden': ([(80, 80)] * 5, 140, True, False, 1, 1),
          'hidden_planes': ([(80, 80)] * 5, 140, False, True, 1, 1)}


def make_batch(B, N, T, lists, codebook):
    c = L.new_batch(B, N, [4, 4, 2, 2, 2])
    c.T, c.n_max, c.n_tiles = T, N, B * -(-N // 16)
    L.point_batch(c, fake(), fake())
    c.code = fake()
    if lists:
        for f in ('mol_info', 'row_ptr', 'col_ptr', 'nbr', 'tnbr', 'ecode', 'tcode', 'blk'):
            setattr(c, f, fake())
        c.build_lists, c.E = 1, 2 * T
    if codebook:
        c.rel_vec[1], c.rel_c[1] = fake(), 3
    return c


def make_layer(structure, training, segs, width):
    p = L.LayerParams()
    p.K, p.structure, p.training = 5, structure, int(training)
    p.inp.nseg = len(segs)
    for i, (w, pad) in enumerate(segs):
        p.inp.width[i], p.inp.pad[i] = w, pad
    p.dropout, p.bn_eps, p.bn_momentum, p.seed = 0.3, 1e-5, 0.1, 7
    for k in range(5):
        p.width[k] = width
        for f in ('att_w', 'self_r', 'W', 'bias', 'gamma', 'beta', 'run_mean', 'run_var'):
            getattr(p, f)[k] = fake()
    p.ave_w = fake() if structure == WEIGHTED else None
    return p


def make_bufs(x, x_planes, aux):
    w = L.LayerBufs()
    for f in ('P', 'Y', 'rscale', 'bn', 'xout', 'pad_row', 'scratch'):
        setattr(w, f, fake())
    w.scratch_bytes = 1 << 40
    w.x = fake() if x else None
    w.x_planes = fake() if x_planes else None
    w.aux_stream = fake() if aux else None
    return w


def expected(structure, batch, layer, mol_grad, training, input_only, has_dx, env):
    """The route, from the description of the policy.  None: not pinned for this call."""
    B, N, T, lists, codebook = BATCHES[batch]
    segs, _, x, x_planes, _, drain_out = LAYERS[layer]
    wt, hidden = structure == WEIGHTED, len(segs) > 1
    mode = env.get('EAGCN_GEMM_X6', '3')
    np_ = hidden and mode in ('3', '4')                         # products from operand planes: hidden layers, plane modes
    gemm3 = hidden and env.get('EAGCN_NO_GEMM3') != '1' and mode != '2'
    force = env.get('EAGCN_BWD_STORE_DH')
    two_pass = wt if force is None else force == '0'            # the second pass re-forms dH (else the first pass stores it)
    wfuse = env.get('EAGCN_LAGG_WFUSE') != '0'
    can_lagg = lists and N <= 256 and env.get('EAGCN_AGG') != 'dense'
    absorbs = (not two_pass) or (wt and wfuse)                  # the LDS-staged kernel would take the second pass
    e = [0] * 16
    e[EDGE_ATOMIC] = int(not codebook)
    e[STORE_DH] = int(not two_pass)
    if T == 0:
        return e
    eval_in = input_only and not training
    if input_only:
        lagg = can_lagg
    else:
        lagg = can_lagg and not codebook and (N >= 240 or absorbs)
    e[FWD_AGG], e[BWD_AGG] = int(can_lagg), int(lagg)
    # (refused: x exists as plane images only and the plane products do not apply)
    e[FWD_PROD] = FWD_PLANES if np_ else FWD_REFUSED if not x else FWD_BALANCED if gemm3 else FWD_TILED
    e[FWD_SPLIT] = int(np_ and not x_planes)
    if eval_in:
        e[BN2] = REDUCE_APPLY if not lagg else STAGED_UPSTREAM if wt else STAGED_ROWMASK
        e[ROWS_FIRST] = int(lagg and mol_grad)
        e[STORE_DH] = None
    elif wt and two_pass and lagg and wfuse:
        e[BN2], e[ROWS_FIRST] = STAGED_UPSTREAM, int(mol_grad)
    elif two_pass:
        e[BN2] = REDUCE_APPLY
    else:
        e[BN2] = STAGED_DH if lagg else ELEMENTWISE
    planes = np_
    e[BWD_SPLIT] = int(planes and not x_planes and not input_only)
    e[PLANES_ONLY] = int(np_)
    if input_only:
        e[BWD_PROD] = PLANES_DX if planes else TILED_DX
        return e
    if not planes and not x:
        e[BWD_PROD] = BWD_REFUSED
        return e
    e[EDGE] = WITH_LAGG if lagg else COLAUNCH
    if planes:
        e[BWD_PROD] = PLANES_PAIR if has_dx else PLANES_DW
    elif gemm3 and has_dx:
        e[BWD_PROD] = G3_SCATTER
    else:
        e[BWD_PROD] = TILED_PAIR if has_dx else TILED_SEPARATE
    e[DEFER] = int(drain_out and not codebook and e[BWD_PROD] == G3_SCATTER)
    return e


def check_invariants(r, training, input_only, x_planes, has_dx, what):
    assert not (r[ROWS_FIRST] and r[ROWS_LATE]), what
    if r[BN2] >= STAGED_DH:
        assert r[BWD_AGG] == 1, what
    if r[EDGE] == WITH_LAGG:
        assert r[EDGE_ATOMIC] == 1 and r[BWD_AGG] == 1, what
    if r[BN2] == STAGED_ROWMASK:
        assert input_only and not training, what
    plane_routes = r[FWD_PROD] == FWD_PLANES and r[BWD_PROD] in (PLANES_PAIR, PLANES_DW, PLANES_DX)
    assert (r[FWD_SPLIT] or r[BWD_SPLIT]) <= (not x_planes), what           # planes that were brought are never formed again
    if x_planes and has_dx:              # the question out[13] answers, asked of a call that brings the planes
        assert bool(r[PLANES_ONLY]) == (plane_routes and not r[FWD_SPLIT] and not r[BWD_SPLIT]), what
    elif r[PLANES_ONLY]:
        assert r[FWD_PROD] == FWD_PLANES, what


# eagcn_layer_{packed, fwd_scratch, bwd_scratch}_bytes with no switch set, as the library returned them BEFORE the carvings
# were folded into one helper (structure does not enter: the scratch is sized by Fp)
SIZES = {
    ('tox21', 'first'): (98560, 23575552, 43406848), ('tox21', 'hidden'): (5899008, 46627072, 118716928),
    ('hiv', 'first'): (98560, 23575552, 133171712), ('hiv', 'hidden'): (5899008, 97023744, 454386688),
    ('no_lists', 'first'): (98560, 23575552, 43406848), ('no_lists', 'hidden'): (5899008, 46627072, 118716928),
    ('n300', 'first'): (98560, 23575552, 49912576), ('n300', 'hidden'): (5899008, 49599744, 142788352),
    ('codebook', 'first'): (98560, 23575552, 43406848), ('codebook', 'hidden'): (5899008, 46627072, 118716928),
    ('empty', 'first'): (98560, 23575552, 17359872), ('empty', 'hidden'): (5899008, 34626304, 32091136),
    ('n256', 'first'): (98560, 23575552, 60881152), ('n256', 'hidden'): (5899008, 54591744, 182761728),
}


def sizes(lib, batch, layer):
    c = make_batch(*BATCHES[batch])
    p = make_layer(CONCATE, True, *LAYERS[layer][:2])
    return tuple(int(f(C.byref(c), C.byref(p))) for f in (lib.eagcn_layer_packed_bytes, lib.eagcn_layer_fwd_scratch_bytes,
                                                           lib.eagcn_layer_bwd_scratch_bytes))


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('EAGCN_')}
    lib = L.load()
    if not env:
        for key, want in SIZES.items():
            got = sizes(lib, *key)
            assert got == want, (key, got, want)
    n = refused = 0
    for structure, batch, layer in itertools.product((CONCATE, WEIGHTED), BATCHES, LAYERS):
        segs, width, x, x_planes, has_dx, drain_out = LAYERS[layer]
        c = make_batch(*BATCHES[batch])
        for mol_grad, training, input_only, aux in itertools.product((0, 1), repeat=4):
            p = make_layer(structure, training, segs, width)
            w = make_bufs(x, x_planes, aux)
            dx = 1 if input_only else has_dx                    # (the input-only form is about dx)
            out = (C.c_int32 * 16)()
            rc = lib.eagcn_layer_route(C.byref(c), C.byref(p), C.byref(w), dx, mol_grad, input_only, drain_out, C.byref(out))
            what = dict(structure=structure, batch=batch, layer=layer, mol_grad=mol_grad, training=training, input_only=input_only,
                        aux=aux, env=env)
            if aux:                                             # the reserved field is set: refused, by name
                assert rc == ERR_ARG and b'aux_stream' in lib.eagcn_last_error(), (what, rc, lib.eagcn_last_error())
                refused += 1
                continue
            assert rc == 0, (what, lib.eagcn_last_error())
            r = list(out)
            want = expected(structure, batch, layer, mol_grad, training, input_only, dx, env)
            diff = {i: (r[i], want[i]) for i in range(16) if want[i] is not None and r[i] != want[i]}
            assert not diff, (what, 'out[i]: (got, want)', diff)
            check_invariants(r, training, input_only, x_planes, dx, what)
            n += 1
    print('routes checked: %d, refusals checked: %d' % (n, refused))


if __name__ == '__main__':
    main()
