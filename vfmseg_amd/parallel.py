"""Data parallelism for the hot path: one process per GPU, torch.distributed over RCCL (backend "nccl" on ROCm),
gloo on CPU for tests.  Replaces mmengine's MMDistributedDataParallel + SyncBatchNorm plumbing
(configs/_base_/default_runtime.py:5, tools/dist_train.sh:9-17).

Only ~16.6 M fp32 gradients (66.5 MB) exist per step, produced in the order VFMHead -> LinearHead -> LoRA layers
L-1..0, and they already sit in ONE flat buffer in that order (optim.FusedAdamW).  The all-reduce is therefore a
handful of large in-place collectives on contiguous slices, issued on a side HIP stream as soon as a slice is
final, overlapping the remaining backward; xGMI is point-to-point so few large buckets beat many small ones.
"""
import os

import torch
import torch.distributed as dist


def single_rank_rehearsal():
    """VFMSEG_DIST_SINGLE=1: run the whole DP plumbing (process group, parameter broadcast, bucketed all-reduce on the side
    stream, SyncBN exchange) with a world of ONE rank.  A box with one GPU cannot host two RCCL ranks, so this is how the `nccl`
    code path itself gets exercised there (tests/test_dp_equivalence_gpu.py); results must equal the non-distributed step."""
    return os.environ.get("VFMSEG_DIST_SINGLE", "0") == "1"


def init_from_env(backend=None):
    """torchrun-style env (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT). Returns (rank, world, local)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if (world > 1 or single_rank_rehearsal()) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = os.environ.get("VFMSEG_DIST_BACKEND", backend)
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def shard_indices(n_total, rank, world, seed=0):
    """mmengine InfiniteSampler: one global shuffled index stream, rank r takes every world-th element."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_total, generator=g).tolist()
    return perm[rank::world]


def broadcast_params(model, src=0):
    """DDP-constructor semantics: rank 0's parameters and buffers win (C3)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not single_rank_rehearsal()):
        return
    for t in list(model.parameters()) + list(model.buffers()):
        dist.broadcast(t.data, src)


# Full fine-tuning: the base weights of DINOv2-L are ~304 M fp32 gradients (1.2 GB), seventy times what the heads and adapters send.
# One bucket would leave nothing to overlap (it is final only when the backward ends); one per block would be 24 collectives whose
# launch and synchronisation cost adds up on a point-to-point fabric where few large transfers beat many small ones (above).  Four
# buckets of whole blocks: three quarters of the traffic leaves while later blocks' backward still runs, each transfer (~300 MB) stays
# far above the size where the collective reaches its bandwidth, and the tail that nothing can hide is one quarter.
MAX_BACKBONE_BUCKETS = 4


def make_buckets(names, offsets, max_lora_buckets=2, max_backbone_buckets=MAX_BACKBONE_BUCKETS):
    """Contiguous [start, end) slices of the flat gradient buffer in production order.
    names/offsets as in FusedAdamW (offsets has len(names)+1 entries).
    The `backbone` family (full fine-tuning) is cut into at most max_backbone_buckets slices `backbone0`, `backbone1`, ... of whole
    blocks, roughly equal in size, last blocks first; the embeddings ride in the last one."""
    from .optim import backbone_block, grad_group
    groups = []
    cur = None
    for i, nm in enumerate(names):
        g = grad_group(nm)
        if g != cur:
            groups.append([g, offsets[i], offsets[i + 1]])
            cur = g
        else:
            groups[-1][2] = offsets[i + 1]
    out = []
    for g, a, b in groups:
        if g == "lora" and max_lora_buckets > 1:
            # split the LoRA run at parameter boundaries into roughly equal halves (layers L-1.. then ..0)
            idx = [i for i, nm in enumerate(names) if "lora_" in nm]
            tgt = (b - a) / max_lora_buckets
            start = a
            k = 1
            for i in idx:
                if offsets[i + 1] - a >= tgt * k and k < max_lora_buckets:
                    out.append((f"lora{k - 1}", start, offsets[i + 1]))
                    start = offsets[i + 1]
                    k += 1
            if start < b:
                out.append((f"lora{k - 1}", start, b))
        elif g == "backbone":
            idx = [i for i, nm in enumerate(names) if grad_group(nm) == "backbone"]
            blocks = sorted({backbone_block(names[i]) for i in idx} - {None}, reverse=True)
            nb = max(1, min(max_backbone_buckets, len(blocks)))
            # the blocks are equal in size: bucket k gets len(blocks) // nb of them (the first len(blocks) % nb buckets one more)
            quota = [len(blocks) // nb + (1 if k < len(blocks) % nb else 0) for k in range(nb)]
            ends = set()      # the block that completes each bucket but the last
            done = 0
            for q in quota[:-1]:
                done += q
                ends.add(blocks[done - 1])
            start, k = a, 0
            for j, i in enumerate(idx):
                # a cut falls only where the next parameter belongs to another block
                nxt = idx[j + 1] if j + 1 < len(idx) else None
                blk = backbone_block(names[i])
                if nxt is not None and blk in ends and backbone_block(names[nxt]) != blk:
                    out.append((f"backbone{k}", start, offsets[i + 1]))
                    start = offsets[i + 1]
                    k += 1
            out.append((f"backbone{k}", start, b))
        else:
            out.append((g, a, b))
    return out


class GradSync:
    """Averaging all-reduce of the flat gradient buffer in production-order buckets.

    `ready(i)` may be called from backward hooks as soon as bucket i is final (overlap on a side stream);
    `finish()` (or calling the object) reduces whatever is still pending and joins the side stream.

    `hold` (set by OptimWrapper before each backward of a gradient-accumulation window that does not end in a step - mmengine's
    no_sync): ready() and finish() send nothing, the gradients stay local and keep adding up; the all-reduce runs once, on the
    micro-step that updates, over the accumulated buffer.  finish() still re-arms the pending-backward count."""

    def __init__(self, gflat, buckets, group=None):
        self.gflat, self.buckets, self.group = gflat, buckets, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (dist.is_initialized() and single_rank_rehearsal())
        self.cuda = gflat.is_cuda
        self.stream = torch.cuda.Stream() if self.cuda else None
        self.done = [False] * len(buckets)
        self.works = []
        self.post_scale = (1.0 / self.world) if self.cuda else 1.0  # consumed by OptimWrapper -> vfm_adamw grad_scale
        self.hold = False
        self.measure = False      # bench.py --gpus N: HIP events around the join in finish() (the all-reduce time backward did not hide)
        self._pairs = []

    def ready(self, i):
        if not self.active or self.hold or self.done[i]:
            return
        _, a, b = self.buckets[i]
        sl = self.gflat[a:b]
        if self.cuda:
            self.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.stream):
                dist.all_reduce(sl, op=dist.ReduceOp.SUM, group=self.group)  # the 1/world average is folded into AdamW
        else:
            self.works.append(dist.all_reduce(sl, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        self.done[i] = True

    def finish(self):
        for i in range(len(self.buckets)):
            self.ready(i)
        if self.active and not self.hold:
            if self.cuda:
                cur = torch.cuda.current_stream()
                if self.measure:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(cur)
                    cur.wait_stream(self.stream)
                    e1.record(cur)
                    self._pairs.append((e0, e1))
                else:
                    cur.wait_stream(self.stream)
            else:
                for w in self.works:
                    w.wait()
                self.works = []
                self.gflat.mul_(1.0 / self.world)
        self.done = [False] * len(self.buckets)
        from . import backbones
        backbones._PENDING_BACKWARD[0] = 0   # (a forward whose backward never ran must not hold the next step's "backbone_done" back)

    __call__ = finish

    def exposed_ms(self):
        """Sum over the measured steps of the time the compute stream stood at the join (call after a device synchronize)."""
        ms = sum(a.elapsed_time(b) for a, b in self._pairs)
        self._pairs = []
        return ms


def bn_sync_fn(group=None):
    """In-place SUM all-reduce used by SyncBatchNorm's moment / gradient exchange (C2)."""
    def f(t):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t
    return f


def attach(model, optim_wrapper, group=None):
    """Wire DP into a built model + OptimWrapper: parameter broadcast, gradient buckets, SyncBN exchange, and the
    backward-time bucket launches (heads' buckets when the backbone backward starts, the first LoRA bucket once the
    blocks it covers are done, the Rein bucket when the backbone backward ends; GradSync.finish() sends the rest and joins
    the side stream)."""
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    if world == 1 and not (dist.is_available() and dist.is_initialized() and single_rank_rehearsal()):
        return None
    broadcast_params(model)
    opt = optim_wrapper.optimizer
    buckets = make_buckets(opt.names, opt.offsets)
    gs = GradSync(opt.gflat, buckets, group)
    optim_wrapper.grad_sync = gs
    from . import backbones
    bb_ids = [i for i, b in enumerate(buckets) if b[0].startswith("backbone")]   # base weights of a fully fine-tuned backbone
    head_ids = [i for i, b in enumerate(buckets) if not b[0].startswith("lora") and b[0] != "reins" and i not in bb_ids]
    rein_ids = [i for i, b in enumerate(buckets) if b[0] == "reins"]   # shared by all layers: final when the backbone backward ends
    lora_ids = [i for i, b in enumerate(buckets) if b[0].startswith("lora")]
    # block index whose completion finalises LoRA bucket k: the smallest block number among the parameters it holds
    last_block = {}
    for i in lora_ids:
        _, a, b = buckets[i]
        blks = [int(nm.split("blocks.")[1].split(".")[0]) for nm, o in zip(opt.names, opt.offsets[:-1]) if a <= o < b and "lora_" in nm]
        last_block[min(blks)] = i
    # the same for the base-weight buckets, except the last one: it holds the embeddings, whose gradients the backward writes last
    from .optim import backbone_block
    for i in bb_ids[:-1]:
        _, a, b = buckets[i]
        blks = [backbone_block(nm) for nm, o in zip(opt.names, opt.offsets[:-1]) if a <= o < b]
        last_block[min(x for x in blks if x is not None)] = i
    rein_ids = rein_ids + bb_ids[-1:]

    def heads_done():
        for i in head_ids:
            gs.ready(i)

    def block_done(li):
        if li in last_block:
            gs.ready(last_block[li])

    def backbone_done():
        for i in rein_ids:
            gs.ready(i)

    backbones.BACKWARD_EVENTS["heads_done"], backbones.BACKWARD_EVENTS["block_done"] = heads_done, block_done
    backbones.BACKWARD_EVENTS["backbone_done"] = backbone_done if rein_ids else None
    head = getattr(model, "decode_head", None)
    for m in (head.modules() if head is not None else []):   # the LinearHead itself, or the one inside an HRDAHead
        if hasattr(m, "bn_sync"):
            m.bn_sync, m.bn_world = bn_sync_fn(group), world
    return gs
