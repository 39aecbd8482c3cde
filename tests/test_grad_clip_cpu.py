"""Host side of gradient clipping / non-finite step skipping (csrc/clip.hip, include/eagcn_hip.h eagcn_grad_norm,
eagcn_adam_step_clipped), no GPU needed: the three entry points are exported and bound, the ABI version did not move, bad arguments
are refused with a message before any HIP call, the workspace size is the header's formula."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('eagcn_grad_norm', 'eagcn_adam_step_clipped', 'eagcn_grad_norm_workspace_bytes')


def _lib():
    import __graft_entry__ as g
    g.build()
    from eagcn_amd import _lib
    return _lib, _lib.load()


def test_entry_points_are_declared_exported_and_bound():
    L, lib = _lib()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = L.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert len(L.SIGNATURES['eagcn_adam_step_clipped'][1]) == len(L.SIGNATURES['eagcn_adam_step'][1]) + 3
    assert lib.eagcn_abi_version() == L.ABI_VERSION == 8


def test_workspace_size_is_the_headers_formula():
    _, lib = _lib()
    text = open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read()
    m = re.search(r'eagcn_grad_norm_workspace_bytes\(\) = (\d+) \+ (\d+) \* (\d+) bytes', text)
    assert m, 'the header documents the workspace size'
    head, slots, slot = (int(x) for x in m.groups())
    assert (head, slots, slot) == (32, 1024, 16)          # 32-byte head, one {double, uint64} per workgroup, at most 1024 of them
    assert lib.eagcn_grad_norm_workspace_bytes() == head + slots * slot


def test_bad_arguments_are_refused_with_a_message():
    """Host memory stands in for device buffers: every call must return before it touches the GPU."""
    _, lib = _lib()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) & ~63                   # 64-byte aligned
    a = [C.c_void_p(base + 256 * i) for i in range(8)]
    odd = C.c_void_p(base + 4)                              # 4-byte aligned only

    def msg():
        return lib.eagcn_last_error()

    # eagcn_grad_norm(grad, live_lanes, n, workspace, accumulate, stream)
    assert lib.eagcn_grad_norm(None, a[1], 8, a[2], 0, None) == -1 and b'null' in msg()
    assert lib.eagcn_grad_norm(a[0], a[1], 8, None, 0, None) == -1 and b'null' in msg()
    assert lib.eagcn_grad_norm(a[0], a[1], 6, a[2], 0, None) == -1 and b'multiple of 4' in msg()
    assert lib.eagcn_grad_norm(a[0], a[1], -4, a[2], 0, None) == -1 and b'multiple of 4' in msg()
    assert lib.eagcn_grad_norm(odd, a[1], 8, a[2], 0, None) == -1 and b'aligned' in msg()
    assert lib.eagcn_grad_norm(a[0], a[1], 8, odd, 0, None) == -1 and b'aligned' in msg()

    # eagcn_adam_step_clipped(param, grad, exp_avg, exp_avg_sq, n, hyper, step, ticket, norm_workspace, clip, stats, stream)
    def step(args, n=8):
        return lib.eagcn_adam_step_clipped(args[0], args[1], args[2], args[3], n, args[4], args[5], args[6], args[7], args[8], args[9], None)
    good = [a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], C.c_void_p(base + 2048), C.c_void_p(base + 2304)]
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9):                  # (6 = the ticket: NULL is a partial update, as with eagcn_adam_step)
        args = list(good)
        args[i] = None
        assert step(args) == -1 and b'null' in msg(), i
    assert step(good, n=10) == -1 and b'multiple of 4' in msg()
    for i in (0, 1, 2, 3, 7):
        args = list(good)
        args[i] = odd
        assert step(args) == -1 and b'aligned' in msg(), i
    for i in (8, 9):
        args = list(good)
        args[i] = odd
        assert step(args) == -1 and b'aligned' in msg(), i
