"""HIP-graph execution of the training step.

The eager engine issues ~60 kernel launches per step; at Tox21 batch sizes the host cannot issue
them as fast as the MI355X retires them.  Every kernel takes its row / tile counts from device
memory and its grid from static capacities, so for a fixed (model, B, N) the launch sequence of the
whole forward and of the whole backward is IDENTICAL from batch to batch: it is captured once into two
HIP graphs and replayed.  What stays eager is only what reads the caller's tensors: the batch-index
kernels (adj / relation tensors) and the packing of ``afms``.  There is no host read-back on the
path; the input-validity counters of batch k are checked (and raised) when batch k+2 is submitted.

Static buffers are sized for ``row_cap`` packed rows (default B*N, which can never overflow).

Everything a batch brings with it is double-buffered (two slots, one captured graph pair each): the
static index, the saved-activation block (whose first region is the packed input), the dropout seeds
and the molecule sizes.  With ``overlap=True`` (inputs already resident in HBM) ALL eager per-batch work
of batch k+1 -- index kernels, packing of ``afms``, seed upload -- runs on a side stream while the GPU is
still executing the backward of batch k; it only has to wait for the backward of batch k-1, the previous
user of its slot.  The main stream then sees nothing but graph launches and the caller's loss.
The captured backward writes the parameter gradients straight into the buffer ``p.grad`` are views of.

The pieces, each written once:
  * ``FlagHandoff`` / ``EventHandoff``: everything that orders the side stream against the step, in its two forms;
  * ``BatchRing``: what the host keeps per batch in flight (pinned validity words, their event, pinned seed staging) and the
    one place that turns it into an error; ``raise_sticky`` for the two sticky words of the library;
  * ``grads_before`` / ``grads_attach``: a step's gradients attached as ``loss.backward()`` would;
  * ``GraphRunner._run``: the one capture site ("first use of a place runs eagerly and is captured, later uses replay") behind
    ``forward``, ``train_step`` and ``attributions``.
graph_composed.ComposedRunner shares the ring and the gradient helper.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from . import ops
from .ops import _index_stream, _ptr, _stream

_RING = 4
# a data-parallel step whose gradient all-reduce cannot be captured into the step graph is an ERROR instead of a (warned)
# fallback to a host-issued collective: bench.py --require-in-graph-allreduce, tools/run_scale.sh
_REQUIRE_IN_GRAPH = os.environ.get('EAGCN_REQUIRE_IN_GRAPH_ALLREDUCE', '0') == '1'
# EAGCN_COMM_IN_GRAPH=0: never try to capture the collective -- the host-issued fallback from the first step on (tests exercise it)
_COMM_IN_GRAPH = os.environ.get('EAGCN_COMM_IN_GRAPH', '1') != '0'
# Capturing a graph that contains collectives, with torch.distributed initialised: the ProcessGroupNCCL watchdog thread polls the
# end events of the EAGER collectives issued before (the warm-up step's all-reduces, the 'dp' loss-scale collective) every 100 ms, and
# an event recorded on the communicator's stream cannot be queried while that stream is part of a capture (hipErrorCapturedEvent:
# "operation not permitted on an event last recorded in a capturing stream") -- the watchdog dies with that exception and takes the
# process with it (SIGABRT; seen in ~1 of 25 runs of tests/dist_multi_check.py: gpurun_out/dist_multi_world1_rc-6.txt).  So the
# eager collectives are allowed to finish AND to be retired by the watchdog before a capture starts: synchronize + this many seconds.
_CAPTURE_DRAIN_S = float(os.environ.get('EAGCN_CAPTURE_DRAIN_S', '0.35'))


# The batch-ready hand-off from the side stream to the step: a device flag that the step's first launch polls
# (eagcn_model.wait_flag) instead of main.wait_event(side event).  hipStreamWaitEvent across two streams costs the waiting stream
# ~40 us per step on ROCm 7.2 even when the event completed long ago (tools/replay_probe.py: 355 us per configs[1] step with
# nothing between the replays, 395 us with an event wait in front of each).  EAGCN_READY_FLAG=0: events.
_READY_FLAG = os.environ.get('EAGCN_READY_FLAG', '1') != '0'
_flag_tested = {}


def _ready_flag_ok(device):
    """Once per device: do the current stream and the index stream really run concurrently?  (Streams that share a hardware queue
    would park the poll in front of its own signal.)  A 50-ms poll on the main stream, the signal on the side stream."""
    if not _READY_FLAG:
        return False
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _flag_tested:
        lib = L.load()
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        torch.cuda.synchronize(device)
        main, side = torch.cuda.current_stream(device), _index_stream(device)
        L.check(lib.eagcn_stream_wait_flag(C.c_void_p(flag.data_ptr()), 0.05, C.c_void_p(main.cuda_stream)), 'eagcn_stream_wait_flag')
        L.check(lib.eagcn_stream_signal_flag(C.c_void_p(flag.data_ptr()), C.c_void_p(side.cuda_stream)), 'eagcn_stream_signal_flag')
        torch.cuda.synchronize(device)
        ok = lib.eagcn_stream_wait_timeouts() == 0
        if not ok:
            import warnings
            lib.eagcn_stream_wait_reset()
            warnings.warn('eagcn_amd: the index stream does not run beside the current stream on this device (shared hardware '
                          'queue?): batch hand-off through stream events instead of a device flag', RuntimeWarning)
        _flag_tested[key] = ok
    return _flag_tested[key]


def _drain_collectives(device):
    """Before capturing a graph in a process with an initialised process group (see _CAPTURE_DRAIN_S)."""
    import torch.distributed as dist
    torch.cuda.synchronize(device)
    if dist.is_available() and dist.is_initialized() and _CAPTURE_DRAIN_S > 0:
        import time
        time.sleep(_CAPTURE_DRAIN_S)


class EventHandoff:
    """What orders the side stream (a batch's preparation) against the main stream (the steps), through stream events; also the
    base of the flag form.  A runner calls, per step: begin() in front of the preparation, ready() behind it, started() once per
    executed forward, forward_done() / step_done() behind it, reset() when a step failed; wire() once per Model struct.  Streams
    and events are only used through wait_event / record / cuda_stream, `new_event` makes an event: a CPU test drives it with fakes.

    Event form: every begin() records an event on the main stream -- its position is "the previous step is done" -- and with
    `overlap` the side stream waits for the event of the begin() BEFORE, behind which the step before the previous one, the last
    user of this batch's slot, is done.  ready() with `overlap` orders the main stream behind an event recorded on the side
    stream; without `overlap` the preparation ran on the main stream and nothing more is recorded or waited for."""

    def __init__(self, new_event):
        self.new_event = new_event
        self.starts = 0                # forwards executed so far (S)
        self.prev = None               # main-stream event of the last begin()
        self.fwd_done = None           # main-stream position behind the last unfused forward graph

    def wire(self, model, slot=None):
        """The hand-off words of `slot` into a Model struct (none: `slot` None, or this form)."""
        model.wait_flag = model.start_signal = None

    def _slot_free(self, main, side, overlap):
        free, self.prev = self.prev, self.new_event()
        self.prev.record(main)
        if overlap and free is not None:
            side.wait_event(free)

    def begin(self, main, side, overlap):
        """In front of a batch's preparation on `side` (= `main` without `overlap`): the slot's last user is done, and the work is
        held back until the FORWARD of the previous unfused step has finished -- from there on the main stream runs the caller's
        loss and the head's backward, short kernels on a few CUs under which the HBM-streaming index scan costs nothing (round 2:
        0.5228 -> 0.5175 ms/step at B = 256, 1.2386 -> 1.2162 at B = 1024 against a start beside the layer GEMMs)."""
        self._slot_free(main, side, overlap)
        if overlap and self.fwd_done is not None:
            side.wait_event(self.fwd_done)

    def ready(self, slot, main, side, overlap):
        """Behind the batch's last preparatory work (torch's copies included) on `side`: the step may consume the slot."""
        if overlap:
            done = self.new_event()
            done.record(side)
            main.wait_event(done)

    def started(self):
        """One executed forward (eager, or a replay of a graph that holds one hand-off-carrying forward)."""
        self.starts += 1

    def forward_done(self, main):
        self.fwd_done = self.new_event()
        self.fwd_done.record(main)

    def step_done(self):
        """A fused step has no launch boundary behind its forward: the next preparation only waits for its slot."""
        self.fwd_done = None

    def reset(self):
        """A step failed between its batch-ready signal and the launch that consumes it (nothing to undo with events)."""


class FlagHandoff(EventHandoff):
    """Flag form.  Per slot a device word "this slot's batch is prepared" (`ready` + 4 * slot), set behind the batch's last
    preparatory kernel (eagcn_stream_signal_flag) and polled and cleared by the step's first launch (eagcn_model.wait_flag).  The
    other direction: every forward adds 1 to the word at `start` in its first launch (eagcn_model.start_signal); when the S-th
    forward issued on the main stream has STARTED, everything issued before it -- the steps that used the slots last -- is done, so
    from S = 2 on the side stream waits for that count (eagcn_stream_wait_counter) instead of for an event recorded on the main
    stream between two step graphs.  `words` reaches the two device words for reset(): synchronize(), zero_ready(), set_start(v)."""

    def __init__(self, new_event, lib, ready, start, words):
        EventHandoff.__init__(self, new_event)
        self.lib, self.ready_word, self.start_word, self.words = lib, int(ready), int(start), words

    def wire(self, model, slot=None):
        model.wait_flag = None if slot is None else self.ready_word + 4 * slot
        model.start_signal = None if slot is None else self.start_word

    def _slot_free(self, main, side, overlap):
        if overlap and self.starts >= 2:
            L.check(self.lib.eagcn_stream_wait_counter(self.start_word, self.starts & 0xFFFFFFFF, side.cuda_stream),
                    'eagcn_stream_wait_counter')

    def ready(self, slot, main, side, overlap):
        L.check(self.lib.eagcn_stream_signal_flag(self.ready_word + 4 * slot, side.cuda_stream), 'eagcn_stream_signal_flag')

    def reset(self):
        """No flag may stay set, and the start word holds the count of the forwards that the host counted."""
        v = self.starts & 0xFFFFFFFF
        self.words.synchronize()
        self.words.zero_ready()
        self.words.set_start(v - 2 ** 32 if v >= 2 ** 31 else v)       # (the count as the int32 device word holds it)
        self.words.synchronize()


class _DeviceWords:
    """The hand-off words of one runner on the device: two ready flags and the start counter (FlagHandoff `words`)."""

    def __init__(self, device):
        self.device = device
        self.ready = torch.zeros(2, dtype=torch.int32, device=device)
        self.start = torch.zeros(1, dtype=torch.int32, device=device)
        self.zero_ready, self.set_start = self.ready.zero_, self.start.fill_

    def synchronize(self):
        torch.cuda.synchronize(self.device)


def _make_handoff(device):
    if not _ready_flag_ok(device):
        return EventHandoff(torch.cuda.Event)
    w = _DeviceWords(device)
    return FlagHandoff(torch.cuda.Event, L.load(), w.ready.data_ptr(), w.start.data_ptr(), w)


def raise_sticky(lib):
    """The two sticky host-mapped words of the library (plain host reads, no synchronisation): the replay loop makes no C call per
    step, so every batch polls them here."""
    if lib.eagcn_stream_wait_timeouts():
        raise L.EagcnHipError('a step waited 2 s for its batch-ready flag (the index stream did not run beside the step: shared '
                              'hardware queue?): results of that step are invalid; set EAGCN_READY_FLAG=0 (stream events) and '
                              'call eagcn_stream_wait_reset()')
    if lib.eagcn_gemm_sk_failed():        # a timed-out stream-K hand-off (csrc/gemm3.hip) poisons its tile
        raise L.EagcnHipError('a stream-K GEMM hand-off timed out in an earlier step (a contributor wave was not '
                              'co-resident with its owner): the gradients of that step are NaN-poisoned; '
                              'eagcn_gemm_sk_reset_failed() clears the flag')


class BatchRing:
    """Per batch in flight, `n` entries: the pinned validity words of its index build (`meta`), the event behind its
    preparation (behind which the words are valid and the staging is free again), whether it came as a bond list (the wording of
    its report) and the pinned staging of its dropout seeds (`seeds`: the source of an asynchronous copy)."""

    def __init__(self, n, row_cap, edge_cap):
        self.row_cap, self.edge_cap = row_cap, edge_cap
        self.meta = [torch.zeros(L.META_WORDS, dtype=torch.int32).pin_memory() for _ in range(n)]
        self.seeds = [torch.zeros(8, dtype=torch.int64).pin_memory() for _ in range(n)]
        self.event = [None] * n
        self.compact = [False] * n

    def filed(self, i, event, compact=False):
        self.event[i], self.compact[i] = event, compact

    def _settle(self, i, prefix):
        """Entry `i` is finished: free it, and raise what its words say against the batch."""
        self.event[i] = None
        bad = L.index_error(self.meta[i].tolist(), self.row_cap, self.edge_cap, self.compact[i])
        if bad:
            raise L.EagcnHipError(prefix + bad)

    def poll(self):
        """The sticky words, and every entry whose batch has finished (no wait)."""
        raise_sticky(L.load())
        for i, ev in enumerate(self.event):
            if ev is not None and ev.query():
                self._settle(i, 'a previous batch: ')

    def free(self, i, prefix='a previous batch: '):
        """Entry `i` is about to be reused: wait for it alone -- the oldest batch in flight.  (Waiting for every entry waits for
        the NEWEST batch's index build too and pulls the host back to less than one step ahead of the GPU every time the ring
        wraps: 38 us of idle main stream per 0.4 ms step at configs[1], profiles/r06_streams_before.txt.)"""
        if self.event[i] is not None:
            self.event[i].synchronize()
            self._settle(i, prefix)

    def check_now(self, i):
        """validate='sync': wait for THIS batch's index kernels and raise before anything consumes the index."""
        self.free(i, '')

    def rows(self, i):
        """Packed rows of entry `i`'s batch (one host wait)."""
        if self.event[i] is not None:
            self.event[i].synchronize()
        return int(self.meta[i][L.META_T])


def grads_before(params, views):
    """In front of a step that OVERWRITES `views` (one per parameter or None: where its gradient will stand): what grads_attach
    needs to attach them as ``loss.backward()`` would.  Returns (todo, kept); `kept` is None when no parameter has a .grad -- the
    usual case after zero_grad(set_to_none), which costs no device work -- and otherwise holds a copy of every view that IS the
    .grad of its parameter (accumulation across steps).  Frozen tensors among `params` (the constant attention weights of
    Vanilla_GCN.hot_params) never get a .grad: zero_grad would not clear it and every later step would accumulate."""
    todo = [(p, v, p.grad) for p, v in zip(params, views) if v is not None and p.requires_grad]
    if all(g is None for _, _, g in todo):
        return todo, None
    return todo, [v.clone() if g is v else None for _, v, g in todo]


def grads_attach(todo, kept):
    if kept is None:
        for p, v, _ in todo:
            p.grad = v
        return
    for (p, v, g), k in zip(todo, kept):
        if g is None:
            p.grad = v
        elif g is v:
            v.add_(k)
        else:
            g.add_(v)                                         # a gradient tensor of the caller's: accumulate into it


class StaticIndex:
    """BatchIndex-compatible view of the runner's static index buffers (capacities, no host values)."""

    def __init__(self, B, N, channels, device, row_cap, edge_cap=None, rel_c=None, structure=-1):
        K = len(channels)
        self.device, self.B, self.N, self.K = device, B, N, K
        self.channels = list(channels)
        self.T = int(row_cap)
        self.n_tiles = B * ((N + 15) // 16)
        self.n_max = N
        c = L.new_batch(B, N, self.channels)
        c.T, c.n_max, c.n_tiles = self.T, N, self.n_tiles
        self.ldc = c.ldc
        blob_lay, rows_lay = L.index_layout(B, N, self.T, self.n_tiles)
        i32 = dict(dtype=torch.int32, device=device)
        self.code = torch.empty((K, B, N, self.ldc), dtype=torch.uint8, device=device)
        blob = torch.zeros(blob_lay['all'].stop, **i32)
        rows = torch.zeros(rows_lay['all'].stop, **i32)
        # bond lists (GAT layers, csrc/gat.hip): capacity in directed bonds; a molecular graph has 2-2.5 per atom
        self.E = int(edge_cap) if edge_cap else min(self.T * N, max(8 * self.T, 1024))
        self._ptrs = torch.zeros(L.bond_ptrs_len(self.T, B), **i32)
        self._edges = torch.zeros(6 * self.E + 2, **i32)       # nbr | tnbr | ecode (u64) | tcode (u64)
        self._blob, self._rows = blob, rows
        self.nat = blob[blob_lay['nat']]
        c.code = self.code.data_ptr()
        L.point_batch(c, blob.data_ptr(), rows.data_ptr(), self._ptrs, self._edges, self.E)
        # bond lists + row blocks: built when the library takes a bond-list form of the aggregation for this shape and layer structure
        # (csrc/lagg.hip); the GAT runner sets the flag itself
        self.bond_lists = bool(L.load().eagcn_agg_wants_bond_lists_for(B, N, int(structure)))
        c.build_lists = 1 if self.bond_lists else 0
        # general relation vectors (layers.py:82 with arbitrary channel values): a static 255-row code book per view
        self.relvec = None
        if rel_c is not None:
            self.relvec = [torch.zeros((255, int(cw)), dtype=torch.float32, device=device) for cw in rel_c]
            for k, t in enumerate(self.relvec):
                c.rel_vec[k], c.rel_c[k] = t.data_ptr(), int(t.shape[1])
        self.c = c

    def ref(self):
        return C.byref(self.c)


class GraphRunner:
    """One captured (forward, backward) pair for a fixed (model plan, B, N, channels); with ``training=False``
    a forward-only graph of the eval-mode model (running BatchNorm statistics, no dropout, no backward)."""

    def __init__(self, plan, B, N, channels, device, dropout, row_cap=None, training=True, static_outputs=False,
                 validate='sync', edge_cap=None, rel_c=None):
        lib = L.load()
        self.plan, self.device = plan, device
        self.training = bool(training)
        self.static_outputs = bool(static_outputs)
        self.validate = validate
        self.key = (B, N, tuple(channels))
        structure = plan.specs[0].structure if getattr(plan, 'specs', None) else -1
        self.slots = [StaticIndex(B, N, channels, device, row_cap if row_cap else B * N, edge_cap, rel_c, structure) for _ in range(2)]
        self.rel_vectors = None        # per batch: the code books of a general batch (set by EAGCN._graph_runner)
        self.index = self.slots[0]
        # captured graphs by place: (slot, 'fwd' | 'bwd' | 'step') or (slot, 'attr', steps, baseline) -> (tag, graph); a place
        # whose tag differs from the one asked for (another loss, optimizer, ...) is captured anew
        self.graphs = {}
        self.dropout = float(dropout)
        self.seeds_dev = [torch.zeros(8, dtype=torch.int64, device=device) for _ in range(2)]
        self.ring = BatchRing(_RING, self.index.T, self.index.E)
        self.step = 0
        self.cur = 0
        self.t_hint = None             # packed rows of the first batch (_set_row_hint): the size hint of every captured launch
        self.n_in = N                  # padded size of the current batch's tensors (EAGCN(n_bucket=...): may be < N)
        self.generation = 0
        self.size_static = [torch.ones(B, dtype=torch.int64, device=device) for _ in range(2)]
        self.dp_group = None
        self.handoff = _make_handoff(device)
        self.use_flag = isinstance(self.handoff, FlagHandoff)  # (read by tools/replay_probe.py and the tests)
        self.cms = [self._cmodel(i) for i in range(2)]
        m = self.cms[0]
        self.saved_bytes = lib.eagcn_model_saved_bytes(self.index.ref(), C.byref(m))
        self.scratch_bytes = lib.eagcn_model_scratch_bytes(self.index.ref(), C.byref(m))
        self.saved = [torch.empty(self.saved_bytes, dtype=torch.uint8, device=device) for _ in range(2)]
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=device)
        if plan.stats is not None:
            from .parallel import register_stats_buffer
            register_stats_buffer(self.scratch)               # (pieces of it are handed to the sync-BatchNorm hook)
        f32 = dict(dtype=torch.float32, device=device)
        self.out = torch.zeros((B, m.head.nclass), **f32)
        self.graph_rep = torch.zeros((B, m.head.n_den2), **f32)
        self.dout = torch.zeros((B, m.head.nclass), **f32)
        self.dgr = torch.zeros((B, m.head.n_den2), **f32)
        self.dgr_is_zero = True
        self._weight_src = None
        # fused training step (forward + loss + backward in ONE graph): labels per slot, class weights, loss value, DP scale
        self.labels_static = [torch.zeros((B, m.head.nclass), **f32) for _ in range(2)]
        self.weight_static = torch.zeros((m.head.nclass, 2), **f32)
        self.loss_static = [torch.zeros((), **f32) for _ in range(2)]
        self.scale_static = [torch.ones((), **f32) for _ in range(2)]      # per slot: written by the NEXT batch's preparation
        self.comm_in_graph = None if _COMM_IN_GRAPH else False   # gradient all-reduce captured inside the step graph (None: not tried yet)
        n = plan.offsets[-1]
        self.flat_acc = torch.zeros(n, **f32)               # the captured backward writes here; p.grad are views of it
        self.acc_views = plan.grad_views(self.flat_acc)
        self.lg, self.hg = plan.grad_structs(self.flat_acc)
        xo, po, ld = C.c_size_t(), C.c_size_t(), C.c_int()
        lib.eagcn_model_atom_rep(self.index.ref(), C.byref(m), C.byref(xo), C.byref(po), C.byref(ld))
        T = self.index.T
        self._xout_views = [sv[xo.value:xo.value + 4 * T * ld.value].view(torch.float32).view(T, ld.value) for sv in self.saved]
        self._pad_views = [sv[po.value:po.value + 4 * ld.value].view(torch.float32) for sv in self.saved]
        self.ptrs = [t.data_ptr() for t in plan._ptr_tensors]
        self._attr = None              # static buffers of atom attributions (attributions(); built on first use)

    def nbytes(self):
        """Device memory this runner holds (two index slots, two saved-activation blocks, scratch, gradients)."""
        n = sum(sv.numel() for sv in self.saved) + self.scratch.numel() + 4 * self.flat_acc.numel()
        for sl in self.slots:
            n += sl.code.numel() + 4 * (sl._blob.numel() + sl._rows.numel() + sl._ptrs.numel() + sl._edges.numel())
        return n

    def release(self):
        """Drop the captured graphs and every static buffer (eviction from EAGCN._runners)."""
        torch.cuda.synchronize(self.device)
        self.graphs = {}
        self.saved, self.scratch, self.slots, self.index = [], None, [], None
        self._xout_views, self._pad_views = [], []
        self._attr = None

    def materializer(self):
        """Callable that builds the current slot's top-layer output matrix (atom representations) when the forward skipped it
        (eagcn_model.fuse_readout); None when the forward builds it.  Valid until the slot's next forward, like the views."""
        if not self.cms[self.cur].fuse_readout:
            return None
        cur, gen = self.cur, self.generation

        def run():
            if self.generation - gen >= 2:
                raise L.EagcnHipError('atom representations of a forward that two newer forwards have overwritten')
            L.check(L.load().eagcn_model_atom_rep_materialize(self.slots[cur].ref(), C.byref(self.cms[cur]), _ptr(self.saved[cur]),
                                                              self.saved_bytes, _stream()), 'eagcn_model_atom_rep_materialize')
        return run

    @property
    def xout_view(self):
        return self._xout_views[self.cur]

    @property
    def pad_view(self):
        return self._pad_views[self.cur]

    # -- C descriptors -------------------------------------------------------------------------------
    def _cmodel(self, slot):
        m = L.Model.from_buffer_copy(self.plan.cmodel(self.training, 0, self.dropout))
        sd = self.seeds_dev[slot].data_ptr()
        for l in range(len(self.plan.layers)):
            m.layer[l].seed_dev = sd + 8 * l
        m.head_seed_dev = sd + 8 * 4
        m.input_packed = 1
        self.handoff.wire(m, slot)
        return m

    def stale(self):
        """Parameter / buffer storage moved (e.g. .to()): the captured pointers are no longer valid."""
        return [t.data_ptr() for t in self.plan._ptr_tensors] != self.ptrs

    # -- the two launch sequences --------------------------------------------------------------------
    def _size_ptr(self):
        """The current slot's molecule sizes (molfp_mode='ave'); null for the sum read-out."""
        return _ptr(self.size_static[self.cur]) if self.plan.molfp else C.c_void_p(0)

    def _call_forward(self):
        L.check(L.load().eagcn_model_forward(self.index.ref(), C.byref(self.cms[self.cur]), C.c_void_p(0), self._size_ptr(),
                                             _ptr(self.saved[self.cur]), self.saved_bytes, _ptr(self.scratch), self.scratch_bytes,
                                             _ptr(self.out), _ptr(self.graph_rep), _stream()), 'eagcn_model_forward')

    def _call_backward(self, with_head=1, hi=None, lo=0):
        """The backward of layers hi .. lo (default: all of them), behind the head's when `with_head`."""
        what = 'eagcn_model_backward' if hi is None else 'eagcn_model_backward_range'
        if hi is None:
            hi = len(self.plan.layers) - 1
        L.check(L.load().eagcn_model_backward_range(self.index.ref(), C.byref(self.cms[self.cur]), self._size_ptr(),
                                                    _ptr(self.saved[self.cur]), self.saved_bytes, _ptr(self.scratch), self.scratch_bytes,
                                                    _ptr(self.dout), _ptr(self.dgr), self.lg, C.byref(self.hg), with_head, hi, lo,
                                                    _stream()), what)

    def _record(self, body):
        """`body` captured into a new graph (nothing executes during capture)."""
        g = torch.cuda.CUDAGraph()
        # thread_local: other threads (e.g. the RCCL watchdog of torch.distributed) may touch the HIP API during capture
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            body()
        return g

    def _run(self, place, body, tag=None, later=None, settle=None):
        """THE capture site.  `body` issues one sequence that holds one hand-off-carrying forward.  First use of `place` (or of
        `place` under this `tag`): the row hint, `body` run eagerly (this call's result, and the warm-up HIP needs before a
        capture), then captured and kept; later uses replay the graph.  Either way one forward has been executed and is counted,
        here and nowhere else; any failure resets the hand-off.  Returns whether this was a first use.

        `later` = (place, body) of a sequence that belongs to the same slot and is replayed by a call of its own (the unfused
        backward): it has never run when the slot is captured, so it is launched once eagerly -- it only overwrites the gradient
        buffer and scratch -- so that no kernel is launched for the first time inside a capture, and is captured behind `body`.
        `settle(failure)`, given when the capture may fail for reasons that are not ours (a collective inside): called with the
        exception of the capture attempt or None; it raises, accepts the graph (None) or returns the (tag, body) to capture
        instead."""
        try:
            ent = self.graphs.get(place)
            first = ent is None or ent[0] != tag
            if not first:
                ent[1].replay()
            else:
                self._set_row_hint()
                body()
                if later is not None:
                    keep = self.flat_acc.clone()              # (gradients of earlier backward passes may be attached to it)
                    later[1]()
                    self.flat_acc.copy_(keep)
                _drain_collectives(self.device)
                L.load().eagcn_prof_enable(0)
                g, failure = None, None
                try:
                    g = self._record(body)
                except Exception as e:                        # noqa: BLE001 -- handed to `settle`
                    if settle is None:
                        raise
                    failure = e
                again = settle(failure) if settle is not None else None
                if again is not None:
                    tag, body = again
                    g = self._record(body)
                self.graphs[place] = (tag, g)
                if later is not None:
                    self.graphs[later[0]] = (None, self._record(later[1]))
            self.handoff.started()
        except BaseException:
            self.handoff.reset()
            raise
        return first

    # -- per-step entry points -----------------------------------------------------------------------
    def _prepare(self, adj, rels, afm, size, seed, overlap=False, bonds=None, labels=None, dp_scale=None):
        """Everything of a step that reads the caller's tensors (index build, packed input, seeds, sizes, labels of a fused
        step), on the side stream when `overlap`; afterwards the main stream is ordered behind it."""
        lib, ring = L.load(), self.ring
        ring.poll()
        self.cur = cur = self.step % 2
        idx = self.index = self.slots[cur]
        main = torch.cuda.current_stream(self.device)
        slot = self.step % _RING
        ring.free(slot)                                       # ring wrapped: this entry must be consumed first
        side = _index_stream(self.device) if overlap else main
        self.handoff.begin(main, side, overlap)
        if overlap:
            for t in (afm, adj, size, labels) + tuple(rels or ()) + tuple(bonds or ()):
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(side)                     # read on the side stream after this call returns
        istream = C.c_void_p(side.cuda_stream)
        idx.c.n_logical = int(self.n_in) if self.n_in != idx.N else 0     # row stride of the caller's tensors / logical N
        # ---- everything that reads the caller's tensors: index, packed input, seeds, sizes -----------------
        ops.index_build(idx.c, adj, rels, bonds, ring.meta[slot], istream, rows=True)
        L.check(lib.eagcn_model_pack_input(idx.ref(), C.byref(self.cms[cur]), _ptr(afm), _ptr(self.saved[cur]),
                                           self.saved_bytes, istream), 'eagcn_model_pack_input')
        sh = ring.seeds[slot]
        sn = sh.numpy()
        sn[:4], sn[4] = L.dropout_seeds(seed)                 # (the derivation of ModelPlan.cmodel: same masks as the eager engine)
        with torch.cuda.stream(side):
            self.seeds_dev[cur].copy_(sh, non_blocking=True)
            if self.plan.molfp:
                self.size_static[cur].copy_(size, non_blocking=True)
            if labels is not None:
                self.labels_static[cur].copy_(labels.reshape(self.labels_static[cur].shape), non_blocking=True)
            if dp_scale is not None:
                if isinstance(dp_scale, str):
                    # c_r = world * n_r / sum_r n_r (parallel.dp_loss_scale) from THIS batch's labels: a 1-element collective
                    # that rides with the batch's preparatory work instead of sitting in front of the step graph
                    from .parallel import dp_loss_scale
                    dp_scale = dp_loss_scale(self.labels_static[cur], self.dp_group)
                self.scale_static[cur].copy_(dp_scale, non_blocking=True)
            if idx.relvec is not None:                       # code books of this batch (rows beyond them are never referenced)
                for t, v in zip(idx.relvec, self.rel_vectors):
                    t[:v.shape[0]].copy_(v, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
        ring.filed(slot, ev, bonds is not None)
        if self.validate == 'sync':
            # (this batch's index kernels only depend on the slot's previous user, not on the main stream's backlog)
            try:
                ring.check_now(slot)
            except L.EagcnHipError:
                if overlap:
                    main.wait_stream(side)
                raise
        self.handoff.ready(cur, main, side, overlap)
        self.step += 1
        self.generation += 1
        if self.training:
            self.plan.nbt_pending += 1    # num_batches_tracked: counted on the host, written by ModelPlan.flush_nbt()
        return main

    def _set_row_hint(self):
        """Before a slot's sequences are captured: tell the library how many packed rows batches of this shape hold (eagcn_batch.t_hint).
        The captured launches are fixed for every later batch of the shape; the buffers are sized for row_cap (default B * N, 7x
        the rows of a Tox21 batch), and the size-dependent kernel choices (the plane GEMM's tile shape, the aggregation form, the
        grid of the bond-list aggregation, the slab layout of the layer scratch) should follow the rows batches of this shape really
        have.  ONE hint per runner -- the rows of the FIRST batch it sees -- for both slots and every kind of captured graph, fixed from
        then on: a slot that captured under another batch's count would freeze other kernels than its twin (even and odd steps would
        differ in timing and rounding).  One host wait, once per runner."""
        if self.t_hint is None:
            t = self.ring.rows((self.step - 1) % _RING)
            self.t_hint = max(1, min(t, self.index.T)) if t > 0 else 0
        for sl in self.slots:
            sl.c.t_hint = self.t_hint

    def forward(self, adj, rels, afm, size, seed, overlap=False, bonds=None):
        main = self._prepare(adj, rels, afm, size, seed, overlap, bonds)
        cur = self.cur
        self._run((cur, 'fwd'), self._call_forward, later=((cur, 'bwd'), self._call_backward) if self.training else None)
        if overlap:
            self.handoff.forward_done(main)
        return self.generation

    def attributions(self, adj, rels, afm, size, dout, steps, baseline, bonds=None):
        """Atom attributions of one eval batch (EAGCN.atom_attributions, graph mode): the whole m-point loop of
        ops.attribution_launches -- pack, forward, input-only backward, accumulate, then finalize -- as ONE captured graph per
        (slot, steps, baseline or not), over static buffers of its own (a scratch block sized for the input backward; the forward
        graphs of the runner keep theirs).  The first call of a key runs the sequence eagerly (the capture warm-up).  Returns fresh
        (score [B, N], attr [B, N, F])."""
        if self.training:
            raise L.EagcnHipError('graph-mode attributions run on the eval runner')
        if self._attr is None:
            m = self.cms[0]
            B, F = self.key[0], int(afm.shape[2])
            a = ops.attribution_buffers(self.index.ref(), m, B, self.key[1], F, self.device)
            a.update(afm=torch.zeros((B, self.key[1], F), dtype=torch.float32, device=self.device), base=torch.zeros_like(afm),
                     dout=torch.zeros((B, m.head.nclass), dtype=torch.float32, device=self.device), models=[])
            self._attr = a
        a = self._attr
        if afm.shape != a['afm'].shape:
            raise L.EagcnHipError('attributions: afms %s, the runner holds %s' % (tuple(afm.shape), tuple(a['afm'].shape)))
        self._prepare(adj, rels, afm, size, 0, False, bonds)         # index + seeds + sizes into the slot; main stream in order
        cur = self.cur
        a['afm'].copy_(afm)
        a['dout'].copy_(dout)
        based = bool(steps and baseline is not None)
        if based:
            a['base'].copy_(baseline)
        # the first forward consumes the slot's ready flag and counts a start like every forward; the others carry no hand-off
        m_first = L.Model.from_buffer_copy(self.cms[cur])
        m_rest = L.Model.from_buffer_copy(self.cms[cur])
        self.handoff.wire(m_rest)
        size_ptr = self._size_ptr()

        def run():
            ops.attribution_launches(self.index.ref(), m_first, m_rest, size_ptr, a['saved'], a['scratch'], a['out'], a['graph_rep'],
                                     a['afm'], a['base'] if based else None, a['dout'], a['acc'], a['attr'], a['score'], steps)
        if self._run((cur, 'attr', int(steps), based), run):
            a['models'] += [m_first, m_rest]                          # (the captured launches read these structs' values at capture)
        return a['score'].clone(), a['attr'].clone()

    def outputs(self):
        """(out, graph_representation) of the last forward.  By default fresh tensors, as the reference returns
        (code that collects predictions / embeddings over several batches, train.py:279-285, keeps working);
        with static_outputs=True views of the static buffers that the next forward of this shape overwrites."""
        if self.static_outputs:
            return self.out.detach(), self.graph_rep.detach()
        return self.out.clone(), self.graph_rep.clone()

    def backward(self, dout, dgr, generation):
        if generation != self.generation:
            raise L.EagcnHipError('graph mode keeps ONE forward in flight: backward() of an older forward was '
                                  'called after a newer training forward overwrote the saved activations')
        if dout.data_ptr() != self.dout.data_ptr():          # the fused losses write straight into self.dout
            self.dout.copy_(dout)
        if dgr is not None:
            self.dgr.copy_(dgr)
            self.dgr_is_zero = False
        elif not self.dgr_is_zero:
            self.dgr.zero_()
            self.dgr_is_zero = True
        # the captured backward OVERWRITES flat_acc (the storage p.grad are views of)
        todo, kept = grads_before(self.plan.params, self.acc_views)
        ent = self.graphs.get((self.cur, 'bwd'))
        if ent is None:
            self._call_backward()
        else:
            ent[1].replay()
        grads_attach(todo, kept)

    # -- fused training step: forward + loss + backward as ONE graph launch -----------------------------
    def _call_forward_step(self, kind, scaled):
        """Forward, loss and the head's backward (eagcn_model_forward_step: the head's eight stages as one launch); the layers'
        backward follows through _call_backward(with_head=0)."""
        cur = self.cur
        sl = L.StepLoss()
        sl.kind = 0 if kind == 'bce' else 1
        sl.labels = self.labels_static[cur].data_ptr()
        sl.class_weight = self.weight_static.data_ptr()
        sl.loss = self.loss_static[cur].data_ptr()
        sl.scale = self.scale_static[cur].data_ptr() if scaled else None       # data-parallel global normalisation (parallel.dp_loss_scale)
        sl.dout = self.dout.data_ptr()
        L.check(L.load().eagcn_model_forward_step(self.index.ref(), C.byref(self.cms[cur]), C.c_void_p(0), self._size_ptr(),
                                                  _ptr(self.saved[cur]), self.saved_bytes, _ptr(self.scratch), self.scratch_bytes,
                                                  _ptr(self.out), _ptr(self.graph_rep), C.byref(sl), _ptr(self.dgr), C.byref(self.hg),
                                                  _stream()), 'eagcn_model_forward_step')

    def _call_backward_comm(self, comm, with_head=1):
        """The backward with the gradient average inside: head + upper layers, then the all-reduce of their bucket of the flat
        gradient buffer is STARTED (asynchronously: under capture a branch of the graph), the first layer's backward runs
        beside it, and its own (small) bucket follows.  One bucket when the model has a single layer."""
        nl = len(self.plan.layers)
        if nl < 2:
            self._call_backward(with_head)
            comm.start(self.flat_acc).wait()
            return
        self._call_backward(with_head, nl - 1, 1)
        cut = self.plan.offsets[self.plan.layer_slices[1][0]]      # first gradient of the second layer: [0, cut) = layer 1
        upper = comm.start(self.flat_acc[cut:])
        self._call_backward(0, 0, 0)
        upper.wait()
        comm.start(self.flat_acc[:cut]).wait()

    def train_step(self, adj, rels, afm, size, seed, labels, kind, weight=None, scale=None, overlap=False, bonds=None,
                   comm=None, optimizer=None):
        """forward -> fused loss (csrc/loss.hip) -> backward of one batch as a single captured graph: no launch boundary
        between the three, one host call per step.  Returns the loss (device scalar); out / graph_representation are read
        with outputs(), the parameter gradients are attached exactly as backward() does.  `comm` (a GradientAllReducer with
        more than one rank behind it): the gradient average is captured into the same graph (_call_backward_comm); should the
        capture of the collective fail on this stack, the runner falls back to one host-issued all-reduce after the replay."""
        if not self.training:
            raise L.EagcnHipError('train_step needs a training-mode runner')
        labels = labels.to(device=self.device, dtype=torch.float32)
        if labels.numel() != self.labels_static[0].numel():
            raise L.EagcnHipError('train_step: %d labels for logits %s' % (labels.numel(), tuple(self.out.shape)))
        if kind == 'bce':
            w = weight.to(device=self.device, dtype=torch.float32)
            if tuple(w.shape) != tuple(self.weight_static.shape):
                raise L.EagcnHipError('bce loss: weight %s for %d tasks' % (tuple(w.shape), self.weight_static.shape[0]))
            tag = (id(w), w._version)
            if self._weight_src != tag:                       # (class weights change once per run, not per step)
                self.weight_static.copy_(w)
                self._weight_src = tag
        if comm is not None and not comm.active():
            comm = None
        self.dp_group = comm.group if comm is not None else None
        if not self.dgr_is_zero:
            self.dgr.zero_()
            self.dgr_is_zero = True
        todo, kept = grads_before(self.plan.params, self.acc_views)
        if optimizer is not None and kept is not None:
            raise L.EagcnHipError('train_step(optimizer=...): the update is part of the step graph and uses this step\'s gradients; '
                                  'call optimizer.zero_grad() (set_to_none) before the step')
        self._prepare(adj, rels, afm, size, seed, overlap, bonds, labels=labels, dp_scale=scale)
        cur, scaled = self.cur, scale is not None
        in_graph = comm is not None and self.comm_in_graph is not False
        # `optimizer` (eagcn_amd.optim.FlatAdam): the parameter update is the last launch of the captured step (its hyper-parameters
        # and step count live in device memory)
        opt_id = id(optimizer) if optimizer is not None else None

        def update():
            if optimizer is not None:
                optimizer.launch(self.flat_acc)

        def body(in_graph=in_graph):
            self._call_forward_step(kind, scaled)
            if in_graph:
                self._call_backward_comm(comm, 0)
            else:
                self._call_backward(0)
                if comm is not None:
                    if torch.cuda.is_current_stream_capturing():
                        return                                # (host-issued average and update behind every replay, below)
                    # eager first use: host-issued average of the flat buffer itself (the .grad views are attached only below: after
                    # zero_grad they are None here and GradientAllReducer.__call__ would find nothing to reduce)
                    comm.start(self.flat_acc).wait()
            update()

        def settle(failure):
            """The capture attempt of a step with the collective inside is over: every rank must replay the SAME collective
            sequence (a rank whose capture failed while the others replay in-graph all-reduces would hang them), so one
            MIN-reduction of the success flag decides for all ranks."""
            if isinstance(failure, L.EagcnHipError):
                comm.agree(False)                             # (the other ranks are waiting in agree() below: fail with them, not hang them)
                raise failure                                 # one of OUR launches failed: never hidden behind a re-capture
            if failure is not None and optimizer is not None:
                optimizer.reset_ticket()                      # (an aborted capture must not leave the update's last-workgroup ticket half counted)
            if comm.agree(failure is None):
                self.comm_in_graph = True
                return None
            if _REQUIRE_IN_GRAPH:
                raise L.EagcnHipError('the gradient all-reduce could not be captured into the step graph on every rank '
                                      '(EAGCN_REQUIRE_IN_GRAPH_ALLREDUCE=1): %r' % (failure,))
            import warnings
            warnings.warn('eagcn_amd: the gradient all-reduce could not be captured into the step graph (%r); falling back '
                          'to one host-issued all-reduce behind every replay' % (failure,), RuntimeWarning)
            # step graph without the collective.  (The eager step left the AVERAGED gradients in the flat buffer; the host-issued
            # average of the first use is then the identity on values that are equal on every rank.)
            _drain_collectives(self.device)
            self.comm_in_graph = False
            return (kind, scaled, False, opt_id), lambda: body(False)

        first = self._run((cur, 'step'), body, (kind, scaled, in_graph, opt_id), settle=settle if in_graph else None)
        self.handoff.step_done()
        grads_attach(todo, kept)
        if comm is not None and not in_graph and not first:
            comm()                                            # one in-place average of the flat buffer, issued by the host
            update()                                          # ... and the update behind it (outside the graph in this fallback)
        return self.loss_static[cur].detach() if self.static_outputs else self.loss_static[cur].clone()


class _GraphFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, adj, rels, afm, size, seed, overlap, trigger, bonds=None):
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[3]:
            raise L.EagcnHipError('graph mode does not produce d/d(afms); use EAGCN.forward_composed for input gradients')
        ctx.runner = runner
        ctx.generation = runner.forward(adj, rels, afm, size, seed, overlap, bonds)
        return runner.outputs()

    @staticmethod
    def backward(ctx, dout, dgr):
        if dout is None:
            dout = torch.zeros_like(ctx.runner.out)
        ctx.runner.backward(dout.contiguous(), None if dgr is None else dgr.contiguous(), ctx.generation)
        return (None,) * 9


def graph_forward(runner, adj, rels, afm, size, seed, overlap=False, bonds=None):
    if not runner.training:               # eval: forward-only graph, nothing to differentiate
        runner.forward(adj, rels, afm, size, seed, overlap, bonds)
        return runner.outputs()
    plan = runner.plan
    if plan.trigger is None or plan.trigger.device != afm.device:
        plan.trigger = torch.zeros((), dtype=torch.float32, device=afm.device, requires_grad=True)
    out, graph_rep = _GraphFn.apply(runner, adj, rels, afm, size, seed, overlap, plan.trigger, bonds)
    out._eagcn_grad_slot = runner.dout    # hints for eagcn_amd.losses: where d(loss)/d(out) is consumed ...
    out._eagcn_step = (runner, runner.generation)      # ... and which captured backward belongs to this forward
    return out, graph_rep
