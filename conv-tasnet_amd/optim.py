"""Flat-buffer optimisers: torch.optim.Adam / torch.optim.SGD semantics on ONE flat fp32 buffer, one HIP kernel pair per step.

Replaces the tail of the reference training step, ``clip_grad_norm_`` + ``optimizer.step()`` over 294 tensors
(src/solver.py:194-196, src/train.py:87-98).  Parameters become views into ``flat_params``; their ``.grad``
are views into ``flat_grads`` -- which is also the single all-reduce payload of the data-parallel step.
``state_dict()`` / ``load_state_dict()`` use torch.optim.Adam's (FlatAdam) and torch.optim.SGD's (FlatSGD) layouts,
so ``optim_dict`` of a reference checkpoint loads here and vice versa.
"""
import torch

from ._lib import lib


def _round4(n):
    return (n + 3) // 4 * 4


class FlatOptimizer(torch.optim.Optimizer):
    """Flat storage shared by FlatAdam and FlatSGD: parameters, their gradients and the optimiser state in flat fp32
    buffers with every tensor 16-byte aligned; one parameter group.  Subclasses add their state (``_alloc_state``) and
    the step."""

    def __init__(self, params, defaults, direct_grads=True):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("%s takes a single parameter group" % type(self).__name__)
        # direct_grads: the HIP backward stages write each parameter gradient straight into flat_grads (no
        # AccumulateGrad add per tensor).  Semantics: a backward pass OVERWRITES the gradient, so accumulate over
        # several backward calls only with direct_grads=False.
        self.direct_grads = bool(direct_grads)
        self._written = set()       # parameters whose sink a backward stage has overwritten since the last zero_grad()
        self._flatten()
        self.last_total_norm = None

    # ---- flat storage -----------------------------------------------------------------
    def _flatten(self):
        name = type(self).__name__
        ps = self.param_groups[0]["params"]
        dev = ps[0].device
        if dev.type != "cuda":
            raise lib_error("%s needs parameters on the GPU (move the model first)" % name)
        self._offsets = []
        off = 0
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("%s: fp32 parameters on one device only" % name)
            self._offsets.append(off)
            off += _round4(p.numel())          # keep every tensor 16-byte aligned for the float4 GEMM loads
        self.numel = off
        self.flat_params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(off, dtype=torch.float32, device=dev)
        self._alloc_state()
        self._ws = torch.empty(lib.ctn_optim_parts(), dtype=torch.float64, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
        for p, o in zip(ps, self._offsets):
            n = p.numel()
            self.flat_params[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat_params[o:o + n].view(p.shape)
            p.grad = self.flat_grads[o:o + n].view(p.shape)
            if self.direct_grads:
                p._ctn_grad_sink = p.grad
                p._ctn_sink_owner = self

    def _alloc_state(self):
        """Allocate the flat optimiser state (self.numel elements per buffer)."""

    def _segments(self):
        """(parameter, offset, numel) of every parameter, in group order."""
        return [(p, o, p.numel()) for p, o in zip(self.param_groups[0]["params"], self._offsets)]

    def _grad_views_intact(self):
        base = self.flat_grads.data_ptr()
        for p, o in zip(self.param_groups[0]["params"], self._offsets):
            if p.grad is None or p.grad.data_ptr() != base + 4 * o:
                return False
        return True

    def zero_grad(self, set_to_none=False):
        """One memset; the .grad views stay attached (set_to_none is ignored on purpose)."""
        gb = getattr(self, "_ctn_buckets", None)
        if gb is not None and (gb.works or gb.covered):
            gb.reset()              # buckets of a backward pass that never reached allreduce_gradients(): parallel.GradientBuckets.reset
        self.flat_grads.zero_()
        self._written.clear()
        if not self._grad_views_intact():
            for p, o in zip(self.param_groups[0]["params"], self._offsets):
                p.grad = self.flat_grads[o:o + p.numel()].view(p.shape)

    def _gather_grads(self):
        """Make flat_grads hold the gradient of this step: gather re-assigned .grad tensors into it, and join the
        weight-gradient stream."""
        if not self._grad_views_intact():      # somebody re-assigned .grad: gather into the flat buffer
            for p, o in zip(self.param_groups[0]["params"], self._offsets):
                seg = self.flat_grads[o:o + p.numel()]
                if p.grad is None:
                    seg.zero_()
                elif p.grad.data_ptr() != seg.data_ptr():
                    seg.copy_(p.grad.reshape(-1))
        from . import ops
        ops.join_side_stream(self.flat_grads.device)      # weight-gradient kernels run on a second stream
        self._written.clear()

    def _group_state(self):
        ps = self.param_groups[0]["params"]
        grp = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(len(ps)))
        return grp


class FlatAdam(FlatOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, direct_grads=True,
                 amsgrad=False, decoupled_weight_decay=False):
        # torch.optim.Adam's checks and messages, before any device work
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError("FlatAdam: amsgrad is not supported")
        if decoupled_weight_decay:
            raise ValueError("FlatAdam: decoupled_weight_decay (AdamW) is not supported; weight_decay is the coupled L2 "
                             "term of torch.optim.Adam")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), direct_grads)
        self._step = 0

    def _alloc_state(self):
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=self.flat_params.device)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=self.flat_params.device)

    # ---- step -------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=0.0, grad_scale=1.0):
        """Adam step; with max_grad_norm > 0 the clip_grad_norm_ rule is fused in front of it.

        grad_scale multiplies the gradient first (1/world after a summing all-reduce).
        The total gradient norm (after grad_scale) is left in ``last_total_norm`` (device scalar).
        weight_decay > 0 adds the coupled L2 term after the clip (ctn_clip_adam_l2_step).

        Non-finite gradients, unlike clip_grad_norm_ (which multiplies every gradient by a NaN or zero coefficient): a NaN
        element makes ``last_total_norm`` NaN and, by C's fminf, the clip coefficient 1, so only that element of the
        parameters and moments turns NaN; an infinite element makes the norm inf and the coefficient 0, so that element
        turns NaN (inf * 0) and every other sees a zero gradient.  Check ``last_total_norm`` to skip such a step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._gather_grads()
        g = self.param_groups[0]
        self._step += 1
        b1, b2 = g["betas"]
        wd = float(g["weight_decay"])
        if wd == 0:
            lib.call("ctn_clip_adam_step", self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(),
                     self.exp_avg_sq.data_ptr(), self.numel, float(grad_scale), float(max_grad_norm), float(g["lr"]),
                     float(b1), float(b2), float(g["eps"]), self._step, self._norm.data_ptr(), self._ws.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        else:
            lib.call("ctn_clip_adam_l2_step", self.flat_params.data_ptr(), self.flat_grads.data_ptr(),
                     self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.numel, float(grad_scale),
                     float(max_grad_norm), float(g["lr"]), float(b1), float(b2), float(g["eps"]), self._step, wd,
                     self._norm.data_ptr(), self._ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        self.last_total_norm = self._norm
        return loss

    # ---- torch.optim.Adam-compatible (de)serialisation -----------------------------------
    def state_dict(self):
        state = {}
        if self._step > 0:
            for i, (p, o, n) in enumerate(self._segments()):
                state[i] = {"step": torch.tensor(float(self._step)),
                            "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        return {"state": state, "param_groups": [self._group_state()]}

    def load_state_dict(self, sd):
        ps = self.param_groups[0]["params"]
        grp = sd["param_groups"][0]
        if grp.get("amsgrad") or grp.get("decoupled_weight_decay"):
            raise ValueError("FlatAdam: cannot load an amsgrad / decoupled_weight_decay (AdamW) state")
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in grp:
                self.param_groups[0][k] = tuple(grp[k]) if k == "betas" else grp[k]
        steps = set()
        for i, (p, o) in enumerate(zip(ps, self._offsets)):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None:
                continue
            n = p.numel()
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("FlatAdam: per-parameter step counts differ")
        self._step = steps.pop() if steps else 0


class FlatSGD(FlatOptimizer):
    """torch.optim.SGD (momentum, dampening, nesterov, coupled weight_decay) on the flat buffers: src/train.py:87-91.

    The momentum buffer is one flat tensor, allocated only when momentum != 0; as in torch the first step after it was
    (re)initialised copies the update instead of decaying a zero buffer."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, direct_grads=True,
                 maximize=False):
        # torch.optim.SGD's checks and messages, before any device work
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if maximize:
            raise ValueError("FlatSGD: maximize is not supported")
        self.momentum_buffer = None
        self._buf_init = False          # False: the next step initialises the buffer with the update (torch's first step)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=False, foreach=None, differentiable=False, fused=None),
                         direct_grads)

    def _alloc_state(self):
        if self.param_groups[0]["momentum"] != 0 and self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros(self.numel, dtype=torch.float32, device=self.flat_params.device)

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=0.0, grad_scale=1.0):
        """SGD step; with max_grad_norm > 0 the clip_grad_norm_ rule is fused in front of it (same contract as
        FlatAdam.step, non-finite gradients included: a NaN element reaches only its own parameter and momentum slot, an
        infinite one zeroes every other gradient of the step).  The hyper-parameters are read from param_groups[0] on every
        call (LR halving edits them)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._gather_grads()
        g = self.param_groups[0]
        mom = float(g["momentum"])
        if mom != 0:
            self._alloc_state()
        buf = self.momentum_buffer.data_ptr() if mom != 0 else 0
        lib.call("ctn_clip_sgd_step", self.flat_params.data_ptr(), self.flat_grads.data_ptr(), buf, self.numel,
                 float(grad_scale), float(max_grad_norm), float(g["lr"]), mom, float(g["dampening"]),
                 float(g["weight_decay"]), int(bool(g["nesterov"])), int(not self._buf_init), self._norm.data_ptr(),
                 self._ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if mom != 0:
            self._buf_init = True
        self.last_total_norm = self._norm
        return loss

    # ---- torch.optim.SGD-compatible (de)serialisation -----------------------------------
    def state_dict(self):
        state = {}
        if self.param_groups[0]["momentum"] != 0 and self._buf_init:
            for i, (p, o, n) in enumerate(self._segments()):
                state[i] = {"momentum_buffer": self.momentum_buffer[o:o + n].view(p.shape).clone()}
        return {"state": state, "param_groups": [self._group_state()]}

    def load_state_dict(self, sd):
        grp = sd["param_groups"][0]
        if grp.get("maximize"):
            raise ValueError("FlatSGD: cannot load a maximize=True state")
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            if k in grp:
                self.param_groups[0][k] = grp[k]
        bufs = []
        for i, (p, o, n) in enumerate(self._segments()):
            st = sd["state"].get(i, sd["state"].get(str(i))) or {}
            bufs.append(st.get("momentum_buffer"))
        have = [b is not None for b in bufs]
        if any(have) and not all(have):
            raise ValueError("FlatSGD: the state holds a momentum buffer for some parameters only")
        self._buf_init = all(have) and bool(have) and self.param_groups[0]["momentum"] != 0
        if self._buf_init:
            self._alloc_state()
            for (p, o, n), b in zip(self._segments(), bufs):
                self.momentum_buffer[o:o + n].copy_(b.reshape(-1))


def lib_error(msg):
    from ._lib import CtnError
    return CtnError(msg)
