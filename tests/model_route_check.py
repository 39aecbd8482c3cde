"""Run by test_host_cpu.py in a subprocess per environment (the library reads its switches once): eagcn_model_route -- the plan of a
whole engine call (csrc/head.hip plan_model: the buffers every layer is handed, its forward and backward route, and what the layers
hand each other) -- over models, batches and calls against plans WRITTEN OUT here from the policy's description (DESIGN.md "the route
of a layer call" and the two "without its reduction pass" sections), never derived from the library.  The routes of the single layer
calls are those of route_check.expected(); what is written here is everything that spans layers.  No GPU: every address is a made-up
multiple of 4096 and nothing is dereferenced."""
import ctypes as C
import os

import route_check as RC

L = RC.L
fake = RC.fake
CONCATE, WEIGHTED = RC.CONCATE, RC.WEIGHTED
STAGED_READOUT = 6
PLANES_ONLY_OUT, SKIP_APPLY, TOP_FORMED, TOP_USED, TOP_GATHER, DH_GIVEN, CARRIES_BELOW, DW_FUSED, WIDE = (1 << i for i in range(9))
ASK_FREE = PLANES_ONLY_OUT | SKIP_APPLY | TOP_FORMED                   # bits the forward acts on: the same whatever the call asks
CUS = 256                                                             # (MI355X; what the library assumes without a device)

TOX21 = (256, 132, 4809, True, False)
# name -> batch (B, N, T, bond lists, code book), structure, view widths per layer, training, read-out mode (0 sum, 1 ave), stats_hook
CASES = {
    'tox21_c2': (TOX21, CONCATE, [80, 140], True, 0, False),
    'tox21_c2_eval': (TOX21, CONCATE, [80, 140], False, 0, False),
    'tox21_c2_ave': (TOX21, CONCATE, [80, 140], True, 1, False),
    'tox21_c3': (TOX21, CONCATE, [80, 140, 140], True, 0, False),
    'tox21_c4': (TOX21, CONCATE, [80, 140, 140, 80], True, 0, False),
    'tox21_w2': (TOX21, WEIGHTED, [80, 140], True, 0, False),
    'odd_widths': (TOX21, CONCATE, [80, 142], True, 0, False),         # 710 read-out columns: no 16-byte gather of the read-out gradient
    'sync_bn': (TOX21, CONCATE, [80, 140], True, 0, True),
    'codebook': ((256, 132, 4809, True, True), CONCATE, [80, 140], True, 0, False),
    'n300': ((64, 300, 6000, False, False), CONCATE, [80, 140], True, 0, False),
    'empty': ((256, 132, 0, True, False), CONCATE, [80, 140], True, 0, False),
}
FORWARD = (0, -1, 0, 0, 0)               # (with_head, layer_hi, layer_lo, has_dx0, input_only): no layer's backward


def asks(n, training):
    top = n - 1
    out = [FORWARD, (1, top, 0, 0, 0), (0, top, 0, 0, 0), (1, top, 0, 1, 0), (1, top, 0, 1, 1), (1, top, 1, 0, 0), (0, 0, 0, 0, 0)]
    if n > 2:
        out += [(1, top, 2, 0, 0), (0, 1, 0, 0, 0)]
    return out


def pad16(w):
    return -(-w // 16) * 16


def by_size_wide(T, ld_in, fp):
    """the pair launch of a plane layer goes to the 256 x 128 kernel from 50 k-tiles (32 deep) of 128 x 128 tiles per CU, dX and dW together"""
    cd = lambda a, b: -(-a // b)
    work = cd(T, 128) * cd(ld_in, 128) * max(1, cd(fp, 32)) + cd(ld_in, 128) * cd(fp, 128) * max(1, cd(T, 32))
    return work >= 50 * CUS


def expected(case, ask, env, top_sw, hidden_sw, first_sw):
    """out[l][0..15] of every layer, from the description of the policy.  None: not pinned."""
    (B, N, T, lists, codebook), structure, widths, training, mode, hook = CASES[case]
    with_head, hi, lo, has_dx0, input_only = ask
    n, top = len(widths), len(widths) - 1
    plane_mode = env.get('EAGCN_GEMM_X6', '3') in ('3', '4')
    concate = structure == CONCATE
    segs = [[(24, 24)]] + [[(w, pad16(w))] * (5 if concate else 1) for w in widths[:-1]]
    ld_in = [sum(p for _, p in s) for s in segs]
    fp = [5 * pad16(w) for w in widths]
    ldo = [f if concate else f // 5 for f in fp]
    # a layer's output also leaves as operand planes when the layer above can run its products from them; it leaves as planes ONLY
    # when that layer then reads nothing else in either direction
    planes_out = [l < top and plane_mode and ldo[l] >= 128 for l in range(n)]
    plane_layer = [plane_mode and ld_in[l] >= 128 for l in range(n)]
    planes_only = [planes_out[l] and plane_layer[l + 1] and T > 0 for l in range(n)]
    RC.BATCHES['model'] = (B, N, T, lists, codebook)

    def route(l, mol_grad, only, has_dx, drain):
        RC.LAYERS['model'] = (segs[l], widths[l], l == 0 or not planes_only[l - 1], l > 0 and planes_out[l - 1], has_dx, drain)
        return RC.expected(structure, 'model', 'model', mol_grad, training, only, has_dx, env)

    # the read-out's sums for the top layer: formed whenever the model qualifies, used unless the call is input-only
    full_top = route(top, 1, 0, int(top > 0), 0)
    formed = (top_sw != 0 and concate and training and not hook and T > 0 and
              full_top[RC.BN2] == RC.STAGED_DH and full_top[RC.EDGE] == RC.WITH_LAGG)
    wide_env = env.get('EAGCN_BX3_WIDE')
    out = []
    carried = False                                  # by the layer above, for the layer about to be described
    for l in range(top, -1, -1):
        fwd = route(l, 0, 0, 0, 0)
        e = [0] * 16
        e[0:3] = fwd[0:3]
        e[13] = int(l > 0 and planes_only[l - 1])
        bits = (PLANES_ONLY_OUT if planes_only[l] else 0) | (SKIP_APPLY if l == top and concate else 0) | (TOP_FORMED if l == top and formed else 0)
        if lo <= l <= hi:
            has_dx = int(l > 0 or has_dx0)
            r = route(l, int(l == top), input_only, has_dx, int(l > lo and not input_only))
            e[3:13] = r[3:13]
            if l == top and formed and not input_only:
                gather = top_sw == 1 and widths[top] % 4 == 0
                e[RC.BN2], e[RC.STORE_DH], e[RC.ROWS_LATE] = STAGED_READOUT, 0, int(not gather)
                bits |= TOP_USED | (TOP_GATHER if gather else 0)
            if carried:
                bits |= DH_GIVEN
            pair = r[RC.BWD_PROD] in (RC.PLANES_PAIR, RC.PLANES_DW)
            wide = pair and (wide_env == '1' or (wide_env != '0' and by_size_wide(T, ld_in[l], fp[l])))
            assert r[RC.BWD_PROD] != RC.PLANES_DW or wide_env in ('0', '1')         # (no such layer here decides by size)
            # the layer below takes dH and its sums from this layer's dX product: a Concate layer in the same call whose reduction pass
            # stores dH for the LDS-staged aggregation, training, local BatchNorm, never more slabs than the pass writes; this layer on
            # the plane pair, 128 x 128 kernel
            carried = False
            if l > lo and not input_only and training and not hook and hidden_sw and concate and T > 0:
                low = route(l - 1, 0, 0, int(l - 1 > 0 or has_dx0), int(l - 1 > lo))
                slabs_pass = max(1, min(-(-(T + 1) // 7), 2048, max(64, (32 << 20) // (fp[l - 1] * 16))))
                carried = (low[RC.BN2] == RC.STAGED_DH and low[RC.STORE_DH] == 1 and -(-T // 64) <= slabs_pass and
                           r[RC.BWD_PROD] == RC.PLANES_PAIR and not wide)
            bits |= (CARRIES_BELOW if carried else 0) | (WIDE if wide else 0)
            # the first layer's weight gradient in the transposed aggregation's epilogue
            if (first_sw and r[RC.BWD_PROD] == RC.TILED_SEPARATE and r[RC.EDGE] == RC.WITH_LAGG and r[RC.BN2] in (RC.STAGED_DH, RC.REDUCE_APPLY) and
                    ld_in[l] <= 32 and env.get('EAGCN_GEMM_X6', '3') not in ('1', '2')):
                bits |= DW_FUSED
                e[15] = None                                      # (at least one slab: checked below)
        e[14] = bits
        out.append(e)
    return out[::-1]


def make_model(case):
    (B, N, T, lists, codebook), structure, widths, training, mode, hook = CASES[case]
    c = RC.make_batch(B, N, T, lists, codebook)
    m = L.Model()
    m.n_layers, m.molfp_mode, m.training, m.fuse_readout, m.stats_world = len(widths), mode, int(training), 1, 1
    concate = structure == CONCATE
    for l, w in enumerate(widths):
        segs = [(24, 24)] if l == 0 else [(widths[l - 1], pad16(widths[l - 1]))] * (5 if concate else 1)
        m.layer[l] = RC.make_layer(structure, training, segs, w)
    h = m.head
    h.f_in, h.n_den1, h.n_den2, h.nclass = (5 * widths[-1] if concate else widths[-1]), 64, 32, 12
    h.dropout, h.bn_eps, h.bn_momentum = 0.3, 1e-5, 0.1
    for f, _ in L.HeadParams._fields_[7:]:
        setattr(h, f, fake())
    if hook:
        m.stats_hook = fake()
    return c, m


def check_invariants(out, n, ask, what):
    with_head, hi, lo, has_dx0, input_only = ask
    for l in range(n):
        o, bits = out[l], out[l][14]
        if l + 1 < n:
            up = out[l + 1]
            planes = up[RC.FWD_PROD] == RC.FWD_PLANES and not up[RC.FWD_SPLIT] and up[13] == 1
            if lo <= l + 1 <= hi:                   # (the backward of the layer above is part of this call)
                planes = planes and up[RC.BWD_PROD] == (RC.PLANES_DX if input_only else RC.PLANES_PAIR) and not up[RC.BWD_SPLIT]
            assert bool(bits & PLANES_ONLY_OUT) == planes, what
            assert bool(bits & DH_GIVEN) == bool(up[14] & CARRIES_BELOW), what
        else:
            assert not bits & (PLANES_ONLY_OUT | DH_GIVEN), what
        assert not (bits & CARRIES_BELOW and bits & WIDE), what
        if bits & TOP_USED:
            assert o[RC.BN2] == STAGED_READOUT and bits & TOP_FORMED, what
        assert bool(bits & TOP_GATHER) <= bool(bits & TOP_USED), what
        assert (o[15] >= 1) == bool(bits & DW_FUSED), what
        if not lo <= l <= hi:
            assert o[3:13] == [0] * 10 and not bits & ~ASK_FREE and o[15] == 0, what


def plan(lib, c, m, ask, saved, scratch):
    out = (C.c_int32 * 16 * 4)()
    rc = lib.eagcn_model_route(C.byref(c), C.byref(m), saved[0], saved[1], scratch[0], scratch[1], *ask, C.byref(out))
    assert rc == 0, (ask, lib.eagcn_last_error())
    return [list(row) for row in out]


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('EAGCN_')}
    lib = L.load()
    checked = 0
    # (top_bn_sums, hidden_bn_sums, first_layer_fused): the defaults, then each setter's other values
    for sw in ((1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 1, 0)):
        old = (lib.eagcn_set_top_bn_sums(sw[0]), lib.eagcn_set_hidden_bn_sums(sw[1]), lib.eagcn_set_first_layer_fused(sw[2]))
        assert old == (1, 1, 1), old
        for case in CASES:
            c, m = make_model(case)
            n = m.n_layers
            saved = (fake(), int(lib.eagcn_model_saved_bytes(C.byref(c), C.byref(m))))
            scratch = (fake() + (1 << 36), int(lib.eagcn_model_scratch_bytes(C.byref(c), C.byref(m))))
            free = None
            for ask in asks(n, CASES[case][3]):
                what = dict(case=case, ask=ask, switches=sw, env=env)
                got = plan(lib, c, m, ask, saved, scratch)
                want = expected(case, ask, env, *sw)
                diff = {(l, i): (got[l][i], want[l][i]) for l in range(n) for i in range(16) if want[l][i] is not None and got[l][i] != want[l][i]}
                assert not diff, (what, 'out[l][i]: (got, want)', diff)
                assert got[n:] == [[0] * 16] * (4 - n), what
                check_invariants(got, n, ask, what)
                now = [got[l][14] & ASK_FREE for l in range(n)] + [got[l][0:3] + got[l][13:14] for l in range(n)]
                assert free is None or free == now, (what, free, now)          # the forward's half: the same whatever the backward asks
                free = now
                checked += 1
        lib.eagcn_set_top_bn_sums(1), lib.eagcn_set_hidden_bn_sums(1), lib.eagcn_set_first_layer_fused(1)
    # a range the engine refuses is refused here, and a block that is too small
    c, m = make_model('tox21_c2')
    out = (C.c_int32 * 16 * 4)()
    big = 1 << 40
    for args in ((fake(), big, fake(), big, 0, 2, 0, 0, 0), (fake(), big, fake(), big, 1, 0, 0, 0, 0), (fake(), 4096, fake(), big, 1, 1, 0, 0, 0),
                 (None, big, fake(), big, 1, 1, 0, 0, 0)):
        assert lib.eagcn_model_route(C.byref(c), C.byref(m), *args, C.byref(out)) == RC.ERR_ARG, args
    print('model plans checked: %d' % checked)


if __name__ == '__main__':
    main()
