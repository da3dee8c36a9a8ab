"""Optimiser side of the hot path: PEFTOptimWrapperConstructor (rein/optimizers/peft_optimizer_constructor.py:18-170),
a fused multi-tensor AdamW over ONE flat fp32 buffer (vfm_adamw) and PolyLR
(configs/dg/gta2citys/dg_lora_dinov2_ms_masked.py:10-29).

All trainable parameters are re-pointed into a flat buffer laid out in gradient-production order
(VFMHead -> LinearHead -> LoRA layers L-1..0), and so are their gradients: the data-parallel all-reduce
(vfmseg_amd.parallel) then works on contiguous bucket slices with no packing copies.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .registry import OPTIM_WRAPPER_CONSTRUCTORS

_NORM_TYPES = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.GroupNorm, nn.LayerNorm)


def param_options(model, base_lr, base_wd, paramwise_cfg):
    """-> {param_name: (lr_mult, weight_decay)} for every trainable parameter, following add_params():
    a custom key (longest first, substring of the full name) wins; otherwise parameters of norm modules get
    weight_decay * norm_decay_mult; everything else (incl. biases, LoRA factors, mask_token) the base values."""
    custom = (paramwise_cfg or {}).get("custom_keys", {})
    keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    norm_decay_mult = (paramwise_cfg or {}).get("norm_decay_mult", None)
    bias_lr_mult = (paramwise_cfg or {}).get("bias_lr_mult", None)
    bias_decay_mult = (paramwise_cfg or {}).get("bias_decay_mult", None)
    out = {}

    def visit(module, prefix):
        is_norm = isinstance(module, _NORM_TYPES)
        for name, p in module.named_parameters(recurse=False):
            if not p.requires_grad:
                continue
            full = f"{prefix}.{name}" if prefix else name
            lr_mult, wd = 1.0, base_wd
            for k in keys:
                if k in f"{prefix}.{name}":
                    lr_mult = custom[k].get("lr_mult", 1.0)
                    wd = base_wd * custom[k].get("decay_mult", 1.0)
                    break
            else:
                if name == "bias" and not is_norm and bias_lr_mult is not None:
                    lr_mult = bias_lr_mult
                if is_norm and norm_decay_mult is not None:
                    wd = base_wd * norm_decay_mult
                elif name == "bias" and bias_decay_mult is not None:
                    wd = base_wd * bias_decay_mult
            out[full] = (lr_mult, wd)
        for cn, child in module.named_children():
            visit(child, f"{prefix}.{cn}" if prefix else cn)

    visit(model, "")
    return out


def is_rein_name(n):
    return n.startswith("reins.") or ".reins." in n


def grad_group(n):
    """Which bucket family a parameter's gradient belongs to (see production_order)."""
    if is_rein_name(n):
        return "reins"
    if "lora_" in n:
        return "lora"
    if n.startswith("backbone."):    # a trained base weight (full fine-tuning): final only when its block's backward has run
        return "backbone"
    return "aux_decoder" if n.startswith("aux_decoder") else "decode_head"


def backbone_block(n):
    """Block index of a base weight's name (`backbone.blocks.N....`), or None for the embeddings (patch_embed / pos_embed / cls_token)."""
    if ".blocks." not in n and not n.startswith("blocks."):
        return None
    try:
        return int(n.split("blocks.")[1].split(".")[0])
    except Exception:
        return None


def production_order(names):
    """Gradient-production order of backward: aux_decoder, decode_head, then LoRA blocks from the last to the first, then the Rein adapter
    (`backbone.reins.*`: weights shared by all layers, whose gradients are complete only when the backbone backward ends).  The base
    weights of a fully fine-tuned backbone (`backbone.*`, neither LoRA nor Rein) follow the heads the same way: blocks from the last to
    the first, then the embeddings, whose gradients are the last thing the backbone backward writes."""
    def key(n):
        if is_rein_name(n):
            return (3, 0, n)
        if grad_group(n) == "backbone":
            blk = backbone_block(n)
            return (4, 1, n) if blk is None else (4, -blk, n)
        if "lora_" in n:
            try:
                blk = int(n.split("blocks.")[1].split(".")[0])
            except Exception:
                blk = 0
            return (2, -blk, n)
        if n.startswith("aux_decoder"):
            return (0, 0, n)
        return (1, 0, n)
    return sorted(names, key=key)


# bumped by every FusedAdamW.step(): caches derived from parameter values (merged LoRA weights for inference) key on it
PARAM_EPOCH = [0]

class PolyLR:
    """mmengine PolyLR(by_epoch=False): lr_t = (base - eta_min) * (1 - t/T)^power + eta_min, t = steps taken."""

    def __init__(self, base_lr, power=0.9, eta_min=0.0, begin=0, end=40000, **kw):
        self.base_lr, self.power, self.eta_min, self.begin, self.end = base_lr, power, eta_min, begin, end

    def lr(self, t):
        t = min(max(t - self.begin, 0), self.end - self.begin)
        return (self.base_lr - self.eta_min) * (1 - t / (self.end - self.begin)) ** self.power + self.eta_min


class FusedAdamW:
    def __init__(self, model, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, paramwise_cfg=None):
        self.lr, self.betas, self.eps = lr, tuple(betas), eps
        opts = param_options(model, lr, weight_decay, paramwise_cfg)
        named = dict(model.named_parameters())
        self.names = production_order([n for n in named if named[n].requires_grad])
        assert set(self.names) == set(opts), "option table / trainable set mismatch"
        self.params = [named[n] for n in self.names]
        dev = self.params[0].device
        sizes = [p.numel() for p in self.params]
        # every parameter starts on a 64-byte boundary of the flat buffers: bias / gamma slices then satisfy the 16-byte
        # operand alignment of the vector GEMM epilogues (a 19-float conv_seg bias used to knock every later bias off it and
        # sent a dozen head GEMMs per step down the scalar epilogue); the pad elements stay zero (zero grad -> zero update)
        self.sizes = sizes
        self.offsets = [0]
        for s in sizes:
            self.offsets.append((self.offsets[-1] + s + 15) // 16 * 16)
        n = self.offsets[-1]
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.gflat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, a, sz in zip(self.params, self.offsets[:-1], sizes):
                b = a + sz
                view = self.flat[a:b].view(p.shape)
                ops.cast(p.detach().reshape(1, -1).contiguous(), self.flat[a:b].view(1, -1))
                p.data = view
                p.grad = self.gflat[a:b].view(p.shape)
                p._vfm_direct_grad = True   # backward kernels accumulate straight into the flat buffer
        self.seg_start = torch.tensor(self.offsets[:-1], dtype=torch.int64, device=dev)
        self.seg_lr = torch.tensor([opts[nm][0] for nm in self.names], dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor([opts[nm][1] for nm in self.names], dtype=torch.float32, device=dev)
        self.step_count = 0
        self.param_groups = [dict(lr=lr)]

    def bucket_slices(self):
        """[(name, start, end)] contiguous gradient slices in production order: aux_decoder, decode_head, lora, reins."""
        cuts, cur = [], None
        for nm, a in zip(self.names, self.offsets[:-1]):
            g = grad_group(nm)
            if g != cur:
                cuts.append([g, a, a])
                cur = g
            cuts[-1][2] = a + dict(zip(self.names, [p.numel() for p in self.params]))[nm]
        return [tuple(c) for c in cuts]

    def step(self, lr=None, grad_scale=1.0, zero_grad=False, skip_flag=None, amp_state=None, clip_coef=None, clip_value=0.0):
        """zero_grad=True clears the flat gradient buffer in the same pass (OptimWrapper.update_params: step, then zero_grad).
        skip_flag / amp_state (AmpOptimWrapper, device tensors): a non-zero flag makes the launch a no-op on parameters and moments;
        with amp_state the loss scale and the step count of the bias corrections are read on the device and `step_count` is the
        wrapper's to maintain (AmpOptimWrapper.sync).
        clip_coef (device scalar: ops.grad_norm's clip state [1:2]) / clip_value: OptimWrapper's clip_grad, consumed inside the launch."""
        if amp_state is None:
            self.step_count += 1
        PARAM_EPOCH[0] += 1  # the fused kernel rewrites the parameters behind torch's version counters
        lr = self.lr if lr is None else lr
        self.param_groups[0]["lr"] = lr
        ops.adamw(self.flat, self.gflat, self.m, self.v, self.seg_start, self.seg_lr, self.seg_wd, lr, self.betas, self.eps,
                  self.step_count, grad_scale, zero_grad=zero_grad, vec4=True, skip=skip_flag, amp_state=amp_state,   # offsets are multiples of 16 floats
                  clip_coef=clip_coef, clip_value=clip_value)
        self._grads_cleared = bool(zero_grad)

    def zero_grad(self):
        if not getattr(self, "_grads_cleared", False):
            self.gflat.zero_()
        self._grads_cleared = False
        for p, a, sz in zip(self.params, self.offsets[:-1], self.sizes):
            if p.grad is None or p.grad.data_ptr() != self.gflat.data_ptr() + a * 4:
                p.grad = self.gflat[a:a + sz].view(p.shape)

    def state_dict(self):
        sync = getattr(self, "_amp_sync", None)
        if sync is not None:   # under AmpOptimWrapper on the GPU the step count lives in the device-side scaler state
            sync()
        return dict(step=self.step_count, m=self.m, v=self.v, names=self.names)

    def load_state_dict(self, sd):
        if list(sd.get("names", self.names)) != list(self.names) or sd["m"].numel() != self.m.numel():
            raise ValueError("optimizer state does not match this model: the flat m/v buffers are laid out by parameter name "
                             f"({len(sd.get('names', []))} saved names / {sd['m'].numel()} elements vs {len(self.names)} / {self.m.numel()})")
        self.step_count = sd["step"]
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])


_INF = float("inf")


def parse_clip_grad(clip_grad):
    """mmengine OptimWrapper's `clip_grad` -> None | dict(type='norm', max_norm, norm_type) | dict(type='value', clip_value).
    'norm' (the default type) is torch.nn.utils.clip_grad_norm_ with norm_type 2 (default), 1 or inf; 'value' is clip_grad_value_.
    What the fused path does not implement is refused by the option's name - never dropped."""
    if clip_grad is None:
        return None
    if not isinstance(clip_grad, dict):
        raise TypeError("optim_wrapper.clip_grad must be None or a dict, got %r" % (clip_grad,))
    cg = dict(clip_grad)
    typ = cg.pop("type", "norm")
    if typ == "value":
        if "clip_value" not in cg:
            raise ValueError("optim_wrapper.clip_grad: type='value' needs clip_value")
        cv = float(cg.pop("clip_value"))
        if cg:
            raise NotImplementedError("optim_wrapper.clip_grad (type='value'): option %r is not supported (clip_value is the only one)" % sorted(cg)[0])
        if not cv > 0:
            raise ValueError("optim_wrapper.clip_grad.clip_value must be > 0, got %r" % (cv,))
        return dict(type="value", clip_value=cv)
    if typ != "norm":
        raise NotImplementedError("optim_wrapper.clip_grad.type=%r ('norm' and 'value' are the two mmengine has)" % (typ,))
    if "max_norm" not in cg:
        raise ValueError("optim_wrapper.clip_grad: type='norm' needs max_norm")
    max_norm = float(cg.pop("max_norm"))
    nt = cg.pop("norm_type", 2)
    if isinstance(nt, str) and nt.lower() in ("inf", "+inf", "infinity"):
        nt = _INF
    if isinstance(nt, bool) or not isinstance(nt, (int, float)) or float(nt) not in (1.0, 2.0, _INF):
        raise NotImplementedError("optim_wrapper.clip_grad.norm_type=%r: the fused norm kernel computes the 2-, 1- and inf-norm" % (nt,))
    if cg.pop("error_if_nonfinite", False):
        raise NotImplementedError("optim_wrapper.clip_grad.error_if_nonfinite=True needs a host read of the norm at every step, which the "
                                  "device-side clipping exists to avoid; read grad_norm() where the check is wanted")
    if cg:
        raise NotImplementedError("optim_wrapper.clip_grad: option %r is not supported (type, max_norm, norm_type, error_if_nonfinite=False)"
                                  % sorted(cg)[0])
    if not max_norm >= 0:   # (a NaN too)
        raise ValueError("optim_wrapper.clip_grad.max_norm must be >= 0, got %r" % (max_norm,))
    return dict(type="norm", max_norm=max_norm, norm_type=float(nt))


class OptimWrapper:
    """mmengine OptimWrapper.update_params: scale_loss -> backward -> [every accumulative_counts-th call: (grad sync) -> clip -> step ->
    zero_grad]; scheduler stepped by iter.

    clip_grad (parse_clip_grad): clipping happens inside step(), on the gradients as the optimiser sees them - after the data-parallel
    average and, under AmpOptimWrapper, after the un-scale.  On the GPU nothing is read back: vfm_grad_norm leaves the norm and the
    coefficient in a 4-float device tensor and the fused AdamW launch takes the coefficient from there; grad_norm() reads the last
    total norm when asked to (one host wait).
    accumulative_counts = N: gradients of N consecutive update_params calls add up in the flat buffer (each loss divided by N, the
    last max_counts % N ones of a run by that remainder), the optimiser steps on every N-th call and on the run's last one.  `iter`
    (the LR schedule) advances on every call, optimizer.step_count (the bias corrections) on real steps only; a step takes the
    schedule's value at the iteration that performs it.  Under data parallelism the held micro-steps send nothing (mmengine's no_sync):
    one set of all-reduces per window, over the accumulated buffer."""

    def __init__(self, optimizer, scheduler=None, grad_sync=None, clip_grad=None, accumulative_counts=1):
        self.optimizer, self.scheduler, self.grad_sync = optimizer, scheduler, grad_sync
        self.iter = 0
        self.clip_grad = parse_clip_grad(clip_grad)
        if isinstance(accumulative_counts, bool) or not isinstance(accumulative_counts, int) or accumulative_counts < 1:
            raise ValueError("optim_wrapper.accumulative_counts must be an integer >= 1, got %r" % (accumulative_counts,))
        self._accumulative_counts = accumulative_counts
        self._inner_count, self._max_counts, self._remainder_counts = 0, -1, -1
        self._clip_state = self._clip_ws = self._clip_flag = None   # device side of the clipping (built at the first GPU step)
        self._host_norm = None

    # ---- gradient accumulation (mmengine OptimWrapper.initialize_count_status / should_update / scale_loss)
    def initialize_count_status(self, init_counts, max_counts):
        """Runner.train: the iteration the run (re)starts at and the one it ends at - the window bookkeeping of accumulative_counts."""
        n = self._accumulative_counts
        self._inner_count, self._max_counts = int(init_counts), int(max_counts)
        if self._inner_count % n != 0:
            import warnings
            warnings.warn(f"Resumed iteration number {init_counts} is not divisible by accumulative_counts={n}: the gradients of the "
                          "window that was open when the checkpoint was written are lost, and the first step comes early")
        residual = self._max_counts - self._inner_count
        self._remainder_counts = residual - residual // n * n

    def should_update(self):
        return self._inner_count % self._accumulative_counts == 0 or self._inner_count == self._max_counts

    def _next_updates(self):
        """Will the backward that is about to run complete a window?  (GradSync is told BEFORE backward: its buckets leave from hooks.)"""
        nxt = self._inner_count + 1
        return nxt % self._accumulative_counts == 0 or nxt == self._max_counts

    def scale_loss(self, loss):
        """mmengine OptimWrapper.scale_loss: loss / accumulative_counts, and in the last max_counts % accumulative_counts iterations of
        a run loss / that remainder; the loss itself when accumulative_counts == 1."""
        n = self._accumulative_counts
        if n == 1:
            return loss
        if self._max_counts != -1 and self._inner_count >= self._max_counts - self._remainder_counts:
            n = self._remainder_counts
            assert n > 0, "update_params called past max_counts"
        return loss / n

    @staticmethod
    def _backward(loss):
        # one device per process: the autograd engine's hand-off to its device thread buys nothing and costs ~15 % of the step's
        # host enqueue time (10.4 vs 12.2 ms of a 15.6-ms step; tools/scratch/_host_profile_step.py)
        with torch.autograd.set_multithreading_enabled(False):
            loss.backward()
        from .functional import join_wgrad_stream
        join_wgrad_stream()   # the heads' weight gradients were issued on a side stream: everything below reads the flat gradient buffer

    def _prepare(self, loss):
        """What backward() runs on: the loss itself (AmpOptimWrapper: times the loss scale)."""
        return loss

    def update_params(self, loss):
        self.backward(self.scale_loss(loss))
        if self.should_update():
            self._step()
            self.optimizer.zero_grad()
        elif self.grad_sync is not None:
            self.grad_sync()   # held (sends nothing): re-arms the buckets and the pending-backward count
        self.iter += 1

    # ---- the piecewise mmengine surface (DACS.train_step: two backward passes, then one step): update_params == backward + step + zero_grad
    def backward(self, loss, **kw):
        """Gradients ACCUMULATE into the flat gradient buffer: a second call before step() adds to the first."""
        if self.grad_sync is not None and self._accumulative_counts != 1:
            self.grad_sync.hold = not self._next_updates()
        self._backward(self._prepare(loss))
        self._inner_count += 1

    def step(self, **kw):
        """What update_params does after its backward, up to and including the fused clearing of the gradients."""
        self._step()
        self.iter += 1

    def _step(self):
        if self.grad_sync is not None:
            self.grad_sync()
        lr = self.scheduler.lr(self.iter) if self.scheduler is not None else None
        post = getattr(self.grad_sync, "post_scale", 1.0)
        self.optimizer.step(lr, grad_scale=post, zero_grad=True, **self._clip(post))

    def zero_grad(self, **kw):
        self.optimizer.zero_grad()

    # ---- clipping
    def _clip(self, pre_scale, amp_state=None, flag=None, host_scale=1.0):
        """-> the keyword arguments the optimiser's step takes for clip_grad ({} when it is off).
        GPU: vfm_grad_norm over the flat buffer (norm of pre_scale [/ amp_state[0]] * g, coefficient and - `flag` - the non-finite flag
        on the device) -> clip_coef for the fused AdamW launch; 'value': clip_value for it.
        Host path (CPU tensors: the stub-optimiser tests): the same semantics from plain torch, applied to the buffer in place."""
        cg = self.clip_grad
        if cg is None:
            return {}
        g = self.optimizer.gflat
        if g.is_cuda:
            if cg["type"] == "value":
                return dict(clip_value=cg["clip_value"])
            if self._clip_state is None or self._clip_state.device != g.device:
                self._clip_state = torch.zeros(4, dtype=torch.float32, device=g.device)
                self._clip_ws = torch.empty(4096, dtype=torch.float64, device=g.device)
            ops.grad_norm(g, cg["norm_type"], cg["max_norm"], pre_scale, amp_state, self._clip_state, flag, self._clip_ws)
            return dict(clip_coef=self._clip_state[1:2])
        s = pre_scale / host_scale
        if cg["type"] == "value":
            g.clamp_(-cg["clip_value"] / s, cg["clip_value"] / s)   # clamp(s g, +-c) = s clamp(g, +-c / s)
            return {}
        total = torch.linalg.vector_norm(g * s, cg["norm_type"])
        self._host_norm = float(total)
        g.mul_(torch.clamp(cg["max_norm"] / (total + 1e-6), max=1.0))   # clip_grad_norm_
        return {}

    def grad_norm(self):
        """Total norm of the gradients of the last step, before clipping, as the optimiser saw them (averaged over ranks, un-scaled);
        None when clip_grad is not type 'norm' or no step has run.  On the GPU this is the one host read clipping ever costs."""
        if self.clip_grad is None or self.clip_grad["type"] != "norm":
            return None
        if self._clip_state is not None:
            return float(self._clip_state[0].item())
        return self._host_norm

    def get_lr(self):
        return self.optimizer.param_groups[0]["lr"]

    def state_dict(self):
        return dict(iter=self.iter)

    def load_state_dict(self, sd):
        self.iter = int(sd.get("iter", self.iter))


class AmpOptimWrapper(OptimWrapper):
    """mmengine AmpOptimWrapper (what tools/train.py:87-102 switches to under `--amp`): the loss is multiplied by a loss scale
    before backward, the gradients are un-scaled inside the optimiser step, a step whose gradients hold an inf / NaN is skipped,
    and with `loss_scale='dynamic'` the scale follows torch.cuda.amp.GradScaler's schedule (init 2**16, x0.5 after a skipped
    step, x2 after `growth_interval` = 2000 consecutive good ones).  A number or a dict(init_scale=, growth_factor=,
    backoff_factor=, growth_interval=) is accepted as in mmengine.

    Autocast dtype (`dtype`, as in mmengine): None / 'float16' = fp16, the CUDA autocast default and what the reference's `--amp`
    runs in - here the precision mode "fp16" (libvfmseg_hip_f16.so: the same kernels with fp16 storage and the fp16 MFMA, fp32
    accumulation, residual stream, statistics and losses); 'bfloat16' = the bf16 mode, where the scale never has to back off in
    practice.  The wrapper records the dtype (`self.dtype`, `self.mode`); the Runner / tools/train.py put the engine into that mode
    (the role of mmengine's optim_context autocast).  The un-scale costs nothing: 1/scale rides on the fused AdamW kernel's grad_scale."""

    _DTYPES = {None: torch.float16, "float16": torch.float16, "fp16": torch.float16, "half": torch.float16, torch.float16: torch.float16,
               "bfloat16": torch.bfloat16, "bf16": torch.bfloat16, torch.bfloat16: torch.bfloat16}

    def __init__(self, optimizer, scheduler=None, grad_sync=None, loss_scale="dynamic", dtype=None, clip_grad=None, accumulative_counts=1):
        super().__init__(optimizer, scheduler, grad_sync, clip_grad=clip_grad, accumulative_counts=accumulative_counts)
        if dtype not in self._DTYPES:
            raise NotImplementedError("AmpOptimWrapper: autocast dtype %r (float16 and bfloat16 are the ones torch.autocast offers on a GPU)" % (dtype,))
        self.dtype = self._DTYPES[dtype]
        self.mode = "fp16" if self.dtype == torch.float16 else "bf16"
        self._tracker, self._skipped = 0, 0
        self._state, self._stale = None, False   # device-side scaler state (built at the first GPU update_params)
        optimizer._amp_sync = self.sync          # FusedAdamW.state_dict() reads the device-side step count back through this
        self.growth_factor, self.backoff_factor, self.growth_interval = 2.0, 0.5, 2000
        self.dynamic = True
        if loss_scale == "dynamic":
            self.scale = 2.0 ** 16
        elif isinstance(loss_scale, dict):
            self.scale = float(loss_scale.get("init_scale", 2.0 ** 16))
            self.growth_factor = float(loss_scale.get("growth_factor", 2.0))
            self.backoff_factor = float(loss_scale.get("backoff_factor", 0.5))
            self.growth_interval = int(loss_scale.get("growth_interval", 2000))
        elif isinstance(loss_scale, (int, float)):
            self.scale, self.dynamic = float(loss_scale), False
        else:
            raise TypeError("loss_scale must be 'dynamic', a number or a dict, got %r" % (loss_scale,))

    def _prepare(self, loss):
        """GradScaler.scale(loss): on the GPU the factor is the DEVICE scale (built here at the first call); every micro-step of an
        accumulation window multiplies by the same one, since the scale moves only in vfm_amp_update, after a step."""
        g = self.optimizer.gflat
        if not g.is_cuda:                    # host path (CPU tensors: tests of the schedule against torch's GradScaler)
            return loss * self._scale
        if self._state is None:
            self._state = torch.tensor([self._scale, float(self._tracker), float(self.optimizer.step_count), float(self._skipped)],
                                       dtype=torch.float32, device=g.device)
        return loss * self._state[0]

    def _step(self):
        """unscale_; [clip]; step (skipped on inf / NaN); update - what follows GradScaler.scale(loss).backward() in update_params.
        On the GPU the scaler's state {scale, growth tracker, optimiser steps, skipped steps} lives in a 4-float DEVICE tensor: the loss
        is multiplied by the device scale, the overflow flag is formed on the device, the fused AdamW launch reads flag, scale and step
        count there (vfm_adamw_guarded) and vfm_amp_update applies GradScaler.update() - the host never waits for the backward pass
        (torch's GradScaler.step pays a found_inf.item() per step with a non-fused optimiser: the host then cannot run ahead of the
        GPU, which cost ~1 ms of a 15.3-ms step here).  `scale`, `skipped`, `growth_tracker` and optimizer.step_count are read back
        on demand (sync()).
        With clip_grad type 'norm' the norm pass (vfm_grad_norm) also forms the flag - one pass over the buffer where
        isfinite(g.sum()) plus a norm would be two - and the norm is that of the UN-SCALED gradients."""
        g = self.optimizer.gflat
        norm_clip = self.clip_grad is not None and self.clip_grad["type"] == "norm"
        if self.grad_sync is not None:
            self.grad_sync()
        post = getattr(self.grad_sync, "post_scale", 1.0)
        lr = self.scheduler.lr(self.iter) if self.scheduler is not None else None
        if not g.is_cuda:
            found_inf = not bool((torch.isfinite(g).all() if norm_clip else torch.isfinite(g.sum())).item())
            flag = torch.tensor([int(found_inf)], dtype=torch.int32)
            self._clip(post, host_scale=self._scale)
            self.optimizer.step(lr, grad_scale=post / self._scale, zero_grad=True, skip_flag=flag)
            if found_inf:
                self._skipped += 1
                self.optimizer.step_count -= 1   # torch's AdamW does not count a skipped step (bias correction)
            self._update_scale(found_inf)
            return
        # after the all-reduce every rank sees the same sums, hence the same decision (an inf / NaN survives the reduction)
        if norm_clip:
            if self._clip_flag is None or self._clip_flag.device != g.device:
                self._clip_flag = torch.zeros(1, dtype=torch.int32, device=g.device)
            flag = self._clip_flag
            kw = self._clip(post, amp_state=self._state, flag=flag)
        else:
            flag = (~torch.isfinite(g.sum())).to(torch.int32).reshape(1)
            kw = self._clip(post)
        self.optimizer.step(lr, grad_scale=post, zero_grad=True, skip_flag=flag, amp_state=self._state, **kw)
        ops.amp_update(flag, self._state, self.growth_factor, self.backoff_factor, self.growth_interval, self.dynamic)
        self._stale = True

    def sync(self):
        """Read the device-side scaler state back (one host wait): scale, growth tracker, skipped steps, optimizer.step_count."""
        if self._stale:
            st = self._state.cpu().tolist()
            self._scale, self._tracker, self._skipped = float(st[0]), int(st[1]), int(st[3])
            self.optimizer.step_count = int(st[2])
            self._stale = False

    def _push(self):
        """The host copies changed (load_state_dict, a scale set by hand): the device tensor is rebuilt at the next update_params."""
        self._state, self._stale = None, False

    @property
    def scale(self):
        self.sync()
        return self._scale

    @scale.setter
    def scale(self, v):
        self.sync()
        self._scale = float(v)
        self._push()

    @property
    def skipped(self):
        self.sync()
        return self._skipped

    @skipped.setter
    def skipped(self, v):
        self.sync()
        self._skipped = int(v)
        self._push()

    @property
    def growth_tracker(self):
        self.sync()
        return self._tracker

    @growth_tracker.setter
    def growth_tracker(self, v):
        self.sync()
        self._tracker = int(v)
        self._push()

    def _update_scale(self, found_inf):
        """torch GradScaler.update(): x backoff after a skipped step, x growth after growth_interval consecutive good ones."""
        if not self.dynamic:
            return
        if found_inf:
            self._scale *= self.backoff_factor
            self._tracker = 0
        else:
            self._tracker += 1
            if self._tracker == self.growth_interval:
                self._scale *= self.growth_factor
                self._tracker = 0

    def state_dict(self):
        self.sync()
        return dict(iter=self.iter, loss_scaler=dict(scale=self.scale, growth_factor=self.growth_factor, backoff_factor=self.backoff_factor,
                                                     growth_interval=self.growth_interval, _growth_tracker=self.growth_tracker))

    def load_state_dict(self, sd):
        # The device-side state of THIS process is dropped first, un-read: reading it back here (the `scale` / `growth_tracker`
        # setters do) would write the old run's step count over the one Runner.resume has just restored into the optimiser.
        self._push()
        super().load_state_dict(sd)
        ls = sd.get("loss_scaler")
        if ls:
            self._scale, self._tracker = float(ls["scale"]), int(ls.get("_growth_tracker", 0))
        # (the device state is rebuilt from the host copies - scale, tracker, optimizer.step_count - at the next update_params)


@OPTIM_WRAPPER_CONSTRUCTORS.register_module()
class PEFTOptimWrapperConstructor:
    def __init__(self, optim_wrapper_cfg, paramwise_cfg=None):
        self.cfg = dict(optim_wrapper_cfg)
        self.cfg.pop("constructor", None)
        self.paramwise_cfg = paramwise_cfg if paramwise_cfg is not None else self.cfg.pop("paramwise_cfg", None)
        self.optimizer_cfg = dict(self.cfg["optimizer"])

    def __call__(self, model, param_scheduler=None):
        model.train()
        oc = dict(self.optimizer_cfg)
        typ = oc.pop("type", "AdamW")
        if typ != "AdamW":
            raise NotImplementedError("the hot path ships the reference's optimiser (AdamW) only")
        opt = FusedAdamW(model, oc.get("lr", 1e-3), oc.get("weight_decay", 0.01), oc.get("betas", (0.9, 0.999)),
                         oc.get("eps", 1e-8), self.paramwise_cfg)
        sched = None
        if param_scheduler:
            sc = dict(param_scheduler[0] if isinstance(param_scheduler, (list, tuple)) else param_scheduler)
            assert sc.pop("type", "PolyLR") == "PolyLR"
            sc.pop("by_epoch", None)
            sched = PolyLR(opt.lr, **sc)
        wtype = self.cfg.get("type", "OptimWrapper")
        common = dict(clip_grad=self.cfg.get("clip_grad"), accumulative_counts=self.cfg.get("accumulative_counts", 1))
        if wtype == "AmpOptimWrapper":
            return AmpOptimWrapper(opt, sched, loss_scale=self.cfg.get("loss_scale", "dynamic"), dtype=self.cfg.get("dtype"), **common)
        if wtype != "OptimWrapper":
            raise NotImplementedError("optim_wrapper type %r (OptimWrapper and AmpOptimWrapper are the ones tools/train.py uses)" % (wtype,))
        return OptimWrapper(opt, sched, **common)
