"""The optimizer step of the reference's training loop (train.py:303 ``optim.Adam(model.parameters(), lr, weight_decay=wd)``,
train.py:334 ``optimizer.step()``) as ONE kernel over ONE flat buffer.

``torch.optim.Adam`` walks ~100 parameter tensors per step (a ``foreach`` pass of a dozen launches).  ``FlatAdam`` re-homes every
hot-path parameter of an ``EAGCN`` into one contiguous fp32 buffer (``p.data`` become views of it, in the order and with the
16-byte alignment of the model's flat gradient buffer, ``ops.ModelPlan.offsets``), keeps the two moment estimates in buffers of
the same layout and updates all of it with ``eagcn_adam_step`` (csrc/loss.hip): same arithmetic as ``torch.optim.Adam`` (L2
``weight_decay`` added to the gradient, bias corrections in double precision).  Hyper-parameters and the step count live in
device memory, so the launch can be captured: ``EAGCN.fused_step(..., optimizer=opt)`` /
``training.train_step(model, opt, ...)`` put it INSIDE the step graph (forward + loss + backward [+ gradient all-reduce] +
update = one graph launch per training step).  Parameters that never receive a gradient (the reference leaves 48 of 177
without one: unused AFM_BatchNorm affine terms, ``self_r`` / ``ave_A`` of the layer wrappers) are not touched, as with
``torch.optim.Adam``, which skips ``grad is None``.

``max_grad_norm`` / ``skip_nonfinite`` (csrc/clip.hip) are ``torch.nn.utils.clip_grad_norm_`` in front of the step and a guard
against NaN / Inf gradients, both on the device: one more launch measures the gradient's 2-norm (fp64, bit-reproducible) and counts
its non-finite elements, the update launch scales the gradient by ``min(1, max_grad_norm / (norm + 1e-6))`` on its way in and, with
``skip_nonfinite``, leaves parameters, moments and the step count alone when there was a NaN / Inf.  Two differences from torch:
the gradient buffer is only READ (``p.grad`` keeps the unclipped values; ``clip_stats()['last_norm']`` is the norm that
``clip_grad_norm_`` would have returned), and a skipped step protects parameters and moments but not the BatchNorm running
statistics, which the forward updated before the gradient existed.
"""
import ctypes as C

import torch

from . import _lib as L


class FlatAdam:
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False):
        if getattr(model, 'structure', None) == 'GAT' or getattr(model, 'molfp_mode', None) == 'pool':
            raise L.EagcnHipError('FlatAdam covers the models with a model-level plan (Concate / Weighted_sum / GCN, sum / ave read-out); '
                                  'use torch.optim.Adam for GAT / pool models')
        self.model = model
        plan = model.plan()
        self.plan = plan
        dev = plan.params[0].device
        if dev.type != 'cuda':
            raise L.EagcnHipError('FlatAdam needs the model on the GPU')
        n = plan.offsets[-1]
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, view in zip(plan.params, plan.grad_views(self.flat)):
                if not p.requires_grad:
                    continue                       # frozen entries of the plan (the constant attention weights of Vanilla_GCN): their
                                                   # slot stays 0 in every buffer, so the kernel's update of it is 0 -= 0
                view.copy_(p.data)
                p.data = view                      # the module's parameter now IS a slice of the flat buffer
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.hyper = torch.tensor([lr, betas[0], betas[1], eps, weight_decay], dtype=torch.float64, device=dev)   # (torch's scalars are doubles)
        self.step_count = torch.zeros((), dtype=torch.int64, device=dev)
        self.ticket = torch.zeros((), dtype=torch.int32, device=dev)
        self._gather = None
        # gradient clipping / non-finite skipping: with both at their defaults launch() is the single eagcn_adam_step; otherwise the
        # norm launch and the clipped update.  Which of the two a captured step graph holds is fixed here, for the optimizer's life.
        self.clipping = max_grad_norm is not None or bool(skip_nonfinite)
        self.max_grad_norm = self._norm_value(max_grad_norm) if max_grad_norm is not None else None
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.clipping:
            lib = L.load()
            self.norm_ws = torch.zeros(int(lib.eagcn_grad_norm_workspace_bytes()) // 8, dtype=torch.int64, device=dev)
            self.clip = torch.tensor([float('inf') if self.max_grad_norm is None else self.max_grad_norm,
                                      1.0 if self.skip_nonfinite else 0.0], dtype=torch.float64, device=dev)
            self.stats = torch.zeros(4, dtype=torch.int64, device=dev)      # applied, skipped, clipped, last_norm (a double's bits)
            # how many leading floats of every group of four are a live gradient: a parameter's elements, not the <= 3 pad words
            # behind them (the weight-gradient epilogues store 16 bytes: a pad word of the gradient buffer holds anything) and not
            # the slot of a frozen parameter
            lanes = torch.zeros(n // 4, dtype=torch.uint8)
            for p, o, k in zip(plan.params, plan.offsets, plan.sizes):
                if p.requires_grad:
                    lanes[o // 4:o // 4 + k // 4] = 4
                    if k % 4:
                        lanes[o // 4 + k // 4] = k % 4
            self.lanes = lanes.to(dev)
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.param_groups = [dict(self.defaults, params=[p for p in plan.params if p.requires_grad])]

    # ---- torch.optim.Optimizer surface the training loop uses -------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        for p in self.param_groups[0]['params']:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def set_lr(self, lr):
        self.hyper[0] = float(lr)                  # (a device write: a captured step graph picks it up at its next replay)
        self.param_groups[0]['lr'] = float(lr)

    @staticmethod
    def _norm_value(x):
        x = float(x)
        if not x > 0.0:                            # (NaN included)
            raise L.EagcnHipError('FlatAdam: max_grad_norm must be a positive number (float(\'inf\') measures without clipping), got %r' % (x,))
        return x

    def set_max_grad_norm(self, max_grad_norm):
        """A device write, like set_lr: a captured step graph reads the new bound at its next replay."""
        if not self.clipping:
            raise L.EagcnHipError('FlatAdam was built without max_grad_norm / skip_nonfinite: its launch (and a step graph that captured '
                                  'it) is the plain eagcn_adam_step; build the optimizer with max_grad_norm=... to clip')
        if max_grad_norm is None:
            raise L.EagcnHipError('FlatAdam: clipping cannot be switched off after construction (the launch sequence is captured); '
                                  'set_max_grad_norm(float(\'inf\')) measures the norm and never clips')
        self.max_grad_norm = self._norm_value(max_grad_norm)
        self.clip[0] = self.max_grad_norm

    def clip_stats(self):
        """{'applied', 'skipped', 'clipped', 'last_norm'}: steps applied, steps skipped for a NaN / Inf gradient, applied steps whose
        gradient was scaled down, and the 2-norm of the last step's gradient before clipping (what ``clip_grad_norm_`` returns; NaN /
        Inf after such a gradient).  One device-to-host copy, which waits for the stream: the only synchronisation of the feature."""
        if not self.clipping:
            raise L.EagcnHipError('FlatAdam.clip_stats(): the optimizer was built without max_grad_norm / skip_nonfinite')
        h = self.stats.cpu()
        return {'applied': int(h[0]), 'skipped': int(h[1]), 'clipped': int(h[2]), 'last_norm': float(h[3:4].view(torch.float64)[0])}

    def reset_ticket(self):
        """After an aborted launch / failed capture: the kernel's last-workgroup ticket starts from zero again (it resets itself at the end
        of every COMPLETED launch; left half counted, later launches would never advance the step count).  Likewise the norm launch's."""
        self.ticket.zero_()
        if self.clipping:
            self.norm_ws[2] = 0                    # (byte 16 of the workspace: the ticket and four reserved bytes)

    def _check_homes(self):
        """The module's parameters must still BE slices of the flat buffer (a later ``model.to()`` / ``.float()`` / assignment to
        ``p.data`` re-homes them and would leave this optimizer updating memory nobody reads)."""
        lo = self.flat.data_ptr()
        hi = lo + 4 * self.flat.numel()
        for p in self.param_groups[0]['params']:
            if not (lo <= p.data_ptr() < hi):
                raise L.EagcnHipError('FlatAdam: a parameter of the model no longer lives in the optimizer\'s flat buffer (the model was moved '
                                      'or a parameter\'s .data was re-assigned after the optimizer was built): build a new FlatAdam')

    def _launch_norm(self, off, n, flat_grad, accumulate):
        L.check(L.load().eagcn_grad_norm(C.c_void_p(flat_grad.data_ptr() + 4 * off), C.c_void_p(self.lanes.data_ptr() + off // 4), n,
                                         C.c_void_p(self.norm_ws.data_ptr()), 1 if accumulate else 0,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'eagcn_grad_norm')

    def _launch(self, off, n, flat_grad, advance):
        lib = L.load()
        if self.clipping:
            L.check(lib.eagcn_adam_step_clipped(C.c_void_p(self.flat.data_ptr() + 4 * off), C.c_void_p(flat_grad.data_ptr() + 4 * off),
                                                C.c_void_p(self.exp_avg.data_ptr() + 4 * off), C.c_void_p(self.exp_avg_sq.data_ptr() + 4 * off),
                                                n, C.c_void_p(self.hyper.data_ptr()), C.c_void_p(self.step_count.data_ptr()),
                                                C.c_void_p(self.ticket.data_ptr()) if advance else C.c_void_p(0),
                                                C.c_void_p(self.norm_ws.data_ptr()), C.c_void_p(self.clip.data_ptr()),
                                                C.c_void_p(self.stats.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'eagcn_adam_step_clipped')
            return
        L.check(lib.eagcn_adam_step(C.c_void_p(self.flat.data_ptr() + 4 * off), C.c_void_p(flat_grad.data_ptr() + 4 * off),
                                    C.c_void_p(self.exp_avg.data_ptr() + 4 * off), C.c_void_p(self.exp_avg_sq.data_ptr() + 4 * off), n,
                                    C.c_void_p(self.hyper.data_ptr()), C.c_void_p(self.step_count.data_ptr()),
                                    C.c_void_p(self.ticket.data_ptr()) if advance else C.c_void_p(0),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'eagcn_adam_step')

    def launch(self, flat_grad):
        """The update as one launch on the current stream (capturable): every slot of the flat buffer has a gradient (graph /
        direct mode: the hot path produces all of them in every backward).  With clipping / skipping: the norm launch, then the
        clipped update (two launches, both capturable)."""
        self._check_homes()
        if self.clipping:
            self._launch_norm(0, self.flat.numel(), flat_grad, False)
        self._launch(0, self.flat.numel(), flat_grad, True)

    @torch.no_grad()
    def step(self):
        flat = self.model.flat_grad_buffer()
        if flat is not None and flat.numel() == self.flat.numel():
            return self.launch(flat)
        # autograd mode: the gradients are separate tensors.  torch.optim.Adam SKIPS a parameter whose .grad is None (no weight decay,
        # no moment update): the parameters that have one are gathered into a staging buffer of the flat layout and updated range by
        # range (adjacent live parameters share a launch); only the last launch advances the step count
        self._check_homes()
        if self._gather is None:
            self._gather = torch.zeros_like(self.flat)
        views = self.plan.grad_views(self._gather)
        offs = self.plan.offsets
        live = [(i, v, p.grad) for i, (v, p) in enumerate(zip(views, self.plan.params)) if p.requires_grad and p.grad is not None]
        if not live:
            return
        torch._foreach_copy_([v for _, v, _ in live], [g for _, _, g in live])
        ranges = []
        for i, _, _ in live:
            if ranges and ranges[-1][1] == offs[i]:
                ranges[-1][1] = offs[i + 1]
            else:
                ranges.append([offs[i], offs[i + 1]])
        if self.clipping:                          # ONE norm over all live ranges (the first launch replaces the totals, the others add)
            for j, (a, b) in enumerate(ranges):
                self._launch_norm(a, b - a, self._gather, j > 0)
        for j, (a, b) in enumerate(ranges):
            self._launch(a, b - a, self._gather, j == len(ranges) - 1)

    def state_dict(self):
        g = self.param_groups[0]
        counts = self.clip_stats() if self.clipping else {'applied': 0, 'skipped': 0, 'clipped': 0}
        return {'max_grad_norm': self.max_grad_norm, 'skip_nonfinite': self.skip_nonfinite,
                'applied': counts['applied'], 'skipped': counts['skipped'], 'clipped': counts['clipped'],
                'exp_avg': self.exp_avg.clone(), 'exp_avg_sq': self.exp_avg_sq.clone(), 'step': int(self.step_count),
                'hyper': self.hyper.clone(),
                # the hyper-parameters as the Python floats they were given as (what load_state_dict restores from)
                'param_group': {'lr': float(g['lr']), 'betas': tuple(float(b) for b in g['betas']), 'eps': float(g['eps']),
                                'weight_decay': float(g['weight_decay'])}}

    def load_state_dict(self, sd):
        """The hyper-parameters are rebuilt in DOUBLE precision from the saved Python floats; a checkpoint that only holds the device
        tensor (older rounds) is taken as it is when it is float64 -- a float32 one (round 4) holds fp32 IMAGES of the values
        (0.99900001287...: exactly the 1.7e-5 error in 1 - beta2 the double hypers exist to avoid), so its entries are rounded
        back to the shortest decimal that has that image.
        One step count for the whole buffer: torch.optim.Adam keeps a count per PARAMETER; with the range-by-range update of the
        autograd mode a parameter whose first gradient arrives in a later step gets the global count's bias correction here.
        Clipping: a dict without the clipping keys, or one saved by an optimizer without clipping, leaves the constructor's
        settings; one saved WITH clipping restores bound, skip flag and counters, and is refused by an optimizer built without."""
        saved_on = sd.get('max_grad_norm') is not None or bool(sd.get('skip_nonfinite', False))
        if saved_on and not self.clipping:
            raise L.EagcnHipError('FlatAdam.load_state_dict: the state was saved with max_grad_norm / skip_nonfinite, this optimizer was '
                                  'built without (clipping cannot be switched on after construction): build it with max_grad_norm=...')
        if saved_on:
            self.skip_nonfinite = bool(sd['skip_nonfinite'])
            self.max_grad_norm = self._norm_value(sd['max_grad_norm']) if sd['max_grad_norm'] is not None else None
            self.clip.copy_(torch.tensor([float('inf') if self.max_grad_norm is None else self.max_grad_norm,
                                          1.0 if self.skip_nonfinite else 0.0], dtype=torch.float64))
            self.stats[:3] = torch.tensor([int(sd.get(k, 0)) for k in ('applied', 'skipped', 'clipped')], dtype=torch.int64)
        self.exp_avg.copy_(sd['exp_avg'])
        self.exp_avg_sq.copy_(sd['exp_avg_sq'])
        self.step_count.fill_(int(sd['step']))
        if 'param_group' in sd:
            g = sd['param_group']
            vals = [g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay']]
        else:
            h = sd['hyper']
            vals = [float(v) for v in h.double().cpu()]
            if h.dtype == torch.float32:
                import numpy as np
                vals = [float(np.format_float_positional(np.float32(v), unique=True, trim='-')) if np.isfinite(v) else v for v in vals]
        self.hyper.copy_(torch.tensor(vals, dtype=torch.float64))
        self.param_groups[0].update(lr=vals[0], betas=(vals[1], vals[2]), eps=vals[3], weight_decay=vals[4])
