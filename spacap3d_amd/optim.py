"""Adam over one flat parameter buffer (csrc/elementwise.hip: adam_flat_kernel; csrc/optim.hip: the grouped mode).

Same update rule as ``torch.optim.Adam(params, lr, weight_decay=wd)`` that the reference builds
(scripts/train.py:262: lr 1e-3, weight_decay 1e-5; L2 decay added to the gradient, bias-corrected moments).  The
parameters that receive gradients are re-pointed at views of ONE flat fp32 buffer (their values are preserved), the
moments are flat buffers of the same size and the step count lives on the device, so an optimizer step is one
gradient pack (``FlatGradBucket.pack``: a multi-tensor copy) + one kernel launch, capturable in the step's hipGraph --
instead of the 8 launches PyTorch's fused multi-tensor Adam needs for the model's ~300 tensors.  The flat gradient
buffer is the one the all-reduce works on, so multi-rank runs pay nothing extra.

Second mode (``groups`` and / or ``max_grad_norm`` given): parameter groups with their own ``lr`` /
``weight_decay`` as the reference builds them (scripts/train.py:226-236), clipping by the global gradient norm
(``torch.nn.utils.clip_grad_norm_``'s formula) and an update that is skipped, not applied, when the gradient is not
finite -- three launches, all hyper-parameters in device memory, no host read.  Without the two arguments nothing changes.

``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s format in both modes.  The index arithmetic between
the flat buffers and per-parameter tensors is in free functions over ``(params, offsets, flat)`` that run on CPU tensors.
"""
import torch

MAX_GROUPS, MAX_SEGMENTS = 8, 4096
# the control record of csrc/optim.hip (include/spacap_hip.h: SPACAP_OPTIM_CTRL_*)
CTRL_COEF, CTRL_APPLY, CTRL_STEP, CTRL_MAX_NORM, CTRL_NORM, CTRL_GROUP_NORM, CTRL_FLOATS = 0, 1, 2, 3, 4, 5, 16


# ---- layout: groups, segments, torch's state indices (plain Python / CPU tensors) -------------------------------------
def normalise_groups(bucket_params, groups, lr, weight_decay):
    """``groups`` (torch-style dicts; missing ``lr`` / ``weight_decay`` default to the arguments) -> (param_groups, group_of):
    ``param_groups`` = [{"params", "lr", "weight_decay"}], ``group_of[i]`` = the group of ``bucket_params[i]``.  Every bucket
    parameter must be in exactly one group; parameters outside the bucket may be listed (they only count for indexing)."""
    if groups is None:
        groups = [{"params": list(bucket_params)}]
    groups = [dict(g) for g in groups]
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"FlatAdam: {len(groups)} parameter groups (1 .. {MAX_GROUPS} supported)")
    owner = {}
    out = []
    for k, g in enumerate(groups):
        unknown = set(g) - {"params", "lr", "weight_decay"}
        if unknown:
            raise ValueError(f"FlatAdam: group {k} has unsupported keys {sorted(unknown)} (per-group lr / weight_decay only)")
        ps = list(g["params"])
        for p in ps:
            if id(p) in owner:
                raise ValueError(f"FlatAdam: a parameter of shape {tuple(p.shape)} appears in groups {owner[id(p)]} and {k}")
            owner[id(p)] = k
        out.append({"params": ps, "lr": float(g.get("lr", lr)), "weight_decay": float(g.get("weight_decay", weight_decay))})
    missing = [tuple(p.shape) for p in bucket_params if id(p) not in owner]
    if missing:
        raise ValueError(f"FlatAdam: {len(missing)} bucket parameters are in no group (shapes {missing[:4]} ...)")
    return out, [owner[id(p)] for p in bucket_params]


def segment_table(offsets, total, group_of):
    """One segment per bucket parameter: (seg_off [S+1] in elements, seg_group [S]).  The padding behind a parameter belongs
    to it.  Offsets must be multiples of 4 (16 bytes): an aligned 16-byte access then never straddles two groups."""
    seg_off = [int(o) for o in offsets] + [int(total)]
    if len(group_of) != len(offsets):
        raise ValueError("segment_table: one group per offset expected")
    if not 1 <= len(offsets) <= MAX_SEGMENTS:
        raise ValueError(f"FlatAdam: {len(offsets)} bucket parameters (1 .. {MAX_SEGMENTS} supported)")
    if seg_off[0] != 0 or any(a > b for a, b in zip(seg_off, seg_off[1:])) or any(o % 4 for o in seg_off[:-1]):
        raise ValueError("segment_table: offsets must start at 0, be sorted and be multiples of 4")
    return seg_off, [int(k) for k in group_of]


def state_index(param_groups):
    """torch's numbering: group by group, each in the order given -> {id(param): index}."""
    idx, n = {}, 0
    for g in param_groups:
        for p in g["params"]:
            idx[id(p)] = n
            n += 1
    return idx


def gather_state(params, offsets, flat):
    """Per-parameter copies of a flat buffer laid out like the bucket (padding dropped)."""
    return [flat[o:o + p.numel()].view(p.shape).clone() for p, o in zip(params, offsets)]


def scatter_state(params, offsets, flat, tensors):
    """The inverse: per-parameter tensors into the flat buffer (padding untouched)."""
    with torch.no_grad():
        for p, o, t in zip(params, offsets, tensors):
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"FlatAdam: state of shape {tuple(t.shape)} for a parameter of shape {tuple(p.shape)}")
            flat[o:o + p.numel()].copy_(t.reshape(-1))


def torch_param_groups(param_groups, betas, eps):
    """``param_groups`` as the installed ``torch.optim.Adam.state_dict()`` writes them (every key it has, at its default)."""
    dicts = [{"params": list(g["params"]), "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in param_groups]
    twin = torch.optim.Adam(dicts, lr=param_groups[0]["lr"], betas=tuple(betas), eps=eps)   # (allocates no state)
    return twin.state_dict()["param_groups"]


def pack_state_dict(param_groups, betas, eps, bucket_params, offsets, m, v, step):
    """``torch.optim.Adam.state_dict()`` for the same ``param_groups``: state entries only for the bucket parameters (the
    others never had a gradient), and none at all before the first update, as in torch."""
    idx = state_index(param_groups)
    state = {}
    if step > 0:
        ms, vs = gather_state(bucket_params, offsets, m), gather_state(bucket_params, offsets, v)
        for p, a, b in zip(bucket_params, ms, vs):
            state[idx[id(p)]] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": a, "exp_avg_sq": b}
        state = dict(sorted(state.items()))
    return {"state": state, "param_groups": torch_param_groups(param_groups, betas, eps)}


def unpack_state_dict(sd, param_groups, bucket_params, offsets, m, v):
    """Writes the moments of ``sd`` into the flat buffers; returns (step, [(lr, weight_decay)] per group).  ``step`` may be
    an int (older torch) or a tensor; all steps must be equal (there is one counter).  Entries of parameters outside the
    bucket are left alone."""
    loaded = sd["param_groups"]
    if len(loaded) != len(param_groups):
        raise ValueError(f"FlatAdam: loaded state dict has {len(loaded)} parameter groups, the optimizer {len(param_groups)}")
    for k, (a, b) in enumerate(zip(loaded, param_groups)):
        if len(a["params"]) != len(b["params"]):
            raise ValueError(f"FlatAdam: loaded group {k} has {len(a['params'])} parameters, the optimizer's {len(b['params'])}")
    # loaded indices -> ours, position by position (torch does the same: the numbers themselves need not match)
    remap = {}
    n = 0
    for a in loaded:
        for i in a["params"]:
            remap[n] = i
            n += 1
    idx = state_index(param_groups)
    state = sd["state"]
    entries = [state.get(remap[idx[id(p)]]) for p in bucket_params]
    have = [e is not None for e in entries]
    if any(have) and not all(have):
        raise ValueError("FlatAdam: the loaded state has entries for some bucket parameters only (their steps would differ)")
    step = 0
    if all(have):
        steps = {float(e["step"]) for e in entries}
        if len(steps) != 1:
            raise ValueError(f"FlatAdam: loaded steps differ ({sorted(steps)[:4]} ...): one step counter for all parameters")
        step = steps.pop()
        if step != int(step) or step < 0:
            raise ValueError(f"FlatAdam: loaded step {step} is not a count")
        for p, e in zip(bucket_params, entries):       # every shape before any write
            for key in ("exp_avg", "exp_avg_sq"):
                if tuple(e[key].shape) != tuple(p.shape):
                    raise ValueError(f"FlatAdam: loaded {key} of shape {tuple(e[key].shape)} for a parameter of shape {tuple(p.shape)}")
        scatter_state(bucket_params, offsets, m, [e["exp_avg"] for e in entries])
        scatter_state(bucket_params, offsets, v, [e["exp_avg_sq"] for e in entries])
    else:
        with torch.no_grad():
            m.zero_()
            v.zero_()
    return int(step), [(float(a["lr"]), float(a["weight_decay"])) for a in loaded]


def reference_order(model):
    """The reference optimizer's two groups (scripts/train.py:226-236): names of the ``requires_grad`` parameters without
    "caption" in their name, then those with, each in ``named_parameters()`` order -> (names, boundary)."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    first = [n for n, _ in named if "caption" not in n]
    second = [n for n, _ in named if "caption" in n]
    return first + second, len(first)


def reference_groups(model, lr, transformer_lr):
    """The same two groups as torch-style dicts over the model's parameters."""
    names, boundary = reference_order(model)
    params = dict(model.named_parameters())
    return [{"params": [params[n] for n in names[:boundary]], "lr": float(lr)},
            {"params": [params[n] for n in names[boundary:]], "lr": float(lr if transformer_lr is None else transformer_lr)}]


@torch.no_grad()
def grad_sqnorm(flat, seg_off, seg_group, num_groups, grad_scale=1.0, max_norm=None):
    """The optimizer's norm pass on its own (two launches, scratch state): ``flat`` f32 [n] on the device, the segment table
    as lists -> (sq f64 [G+1]: per group then total, norms f32 [G+1]: grad_scale * sqrt(sq), coef f32 scalar), all on the
    device, nothing read back."""
    from ._native import check, lib
    if not flat.is_cuda:
        raise RuntimeError("CPU not supported")
    dev, n, S, G = flat.device, flat.numel(), len(seg_group), int(num_groups)
    off_h, grp_h = torch.tensor(list(seg_off), dtype=torch.int64), torch.tensor(list(seg_group), dtype=torch.int32)
    if off_h.numel() != S + 1:
        raise ValueError("grad_sqnorm: seg_off must have one more entry than seg_group")
    off_d, grp_d = off_h.to(dev), grp_h.to(dev)
    blocks = int(lib.spacap_optim_blocks(n))
    partials = torch.zeros(max(blocks, 1), max(G, 1), dtype=torch.float64, device=dev)
    sq = torch.zeros(G + 1, dtype=torch.float64, device=dev)
    ctrl = torch.zeros(CTRL_FLOATS, dtype=torch.float32, device=dev)
    if max_norm is not None:
        ctrl[CTRL_MAX_NORM] = float(max_norm)
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib.spacap_grad_sqnorm_f32(flat.data_ptr(), n, off_d.data_ptr(), grp_d.data_ptr(), S, G, off_h.data_ptr(),
                                         grp_h.data_ptr(), partials.data_ptr(), stream), "spacap_grad_sqnorm_f32")
        check(lib.spacap_optim_finish_f64(partials.data_ptr(), blocks, G, float(grad_scale), None, sq.data_ptr(),
                                          ctrl.data_ptr(), skipped.data_ptr(), stream), "spacap_optim_finish_f64")
    norms = torch.cat([ctrl[CTRL_GROUP_NORM:CTRL_GROUP_NORM + G], ctrl[CTRL_NORM:CTRL_NORM + 1]])
    return sq, norms, ctrl[CTRL_COEF].clone()


class FlatAdam:
    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, groups=None, max_grad_norm=None):
        self.bucket = bucket
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        flat_g = bucket.flat
        if not flat_g.is_cuda:
            raise RuntimeError("CPU not supported")
        self.grouped = groups is not None or max_grad_norm is not None
        self.param_groups, group_of = normalise_groups(bucket.params, groups, self.lr, self.weight_decay)
        if self.grouped:
            seg_off, seg_group = segment_table(bucket.offsets, flat_g.numel(), group_of)
        self.flat_p = torch.zeros_like(flat_g)
        with torch.no_grad():
            for p, off in zip(bucket.params, bucket.offsets):   # same (16-byte aligned) layout as the gradient bucket
                view = self.flat_p[off:off + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view          # the module's parameter now lives in the flat buffer
        self.m = torch.zeros_like(flat_g)
        self.v = torch.zeros_like(flat_g)
        if not self.grouped:
            self.step_t = torch.zeros((), dtype=torch.float32, device=flat_g.device)
            return
        from ._native import lib
        dev = flat_g.device
        G = len(self.param_groups)
        # host copies (checked by the entry points at every call) and the device tables the kernels read
        self._seg_off_host = torch.tensor(seg_off, dtype=torch.int64)
        self._seg_group_host = torch.tensor(seg_group, dtype=torch.int32)
        self._seg_off, self._seg_group = self._seg_off_host.to(dev), self._seg_group_host.to(dev)
        self._hyper = torch.tensor([[g["lr"], g["weight_decay"]] for g in self.param_groups], dtype=torch.float32).to(dev)
        self._ctrl = torch.zeros(CTRL_FLOATS, dtype=torch.float32, device=dev)
        self._ctrl[CTRL_COEF] = 1.0
        self._blocks = int(lib.spacap_optim_blocks(flat_g.numel()))
        self._partials = torch.zeros(self._blocks, G, dtype=torch.float64, device=dev)
        self.grad_sqnorm = torch.zeros(G + 1, dtype=torch.float64, device=dev)   # per group, then the total (of bucket.flat, unscaled)
        self._skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        # telemetry: device tensors, rewritten by every step, static under graph replay
        self.step_t = self._ctrl[CTRL_STEP]
        self.clip_coef = self._ctrl[CTRL_COEF]
        self.grad_norm = self._ctrl[CTRL_NORM]
        self.group_grad_norm = self._ctrl[CTRL_GROUP_NORM:CTRL_GROUP_NORM + G]
        self.skipped_updates = self._skipped[0]
        self.max_grad_norm = None
        self.set_max_grad_norm(max_grad_norm)

    # -- hyper-parameters in device memory (grouped mode): no kernel argument changes, a captured graph keeps working ----
    def _need_grouped(self, what):
        if not self.grouped:
            raise RuntimeError(f"FlatAdam.{what} needs the grouped mode (build it with groups= and / or max_grad_norm=)")

    @torch.no_grad()
    def _write_hyper(self):
        host = torch.tensor([[g["lr"], g["weight_decay"]] for g in self.param_groups], dtype=torch.float32)
        self._hyper.copy_(host)          # stream-ordered: the next launch (or graph replay) on this stream reads the new rates

    def set_lr(self, lr=None, group_lrs=None):
        """``lr``: one rate for every group; ``group_lrs``: one per group (None entries keep theirs)."""
        self._need_grouped("set_lr")
        if lr is not None:
            self.lr = float(lr)
            for g in self.param_groups:
                g["lr"] = float(lr)
        if group_lrs is not None:
            if len(group_lrs) != len(self.param_groups):
                raise ValueError(f"FlatAdam.set_lr: {len(group_lrs)} rates for {len(self.param_groups)} groups")
            for g, x in zip(self.param_groups, group_lrs):
                if x is not None:
                    g["lr"] = float(x)
        self._write_hyper()

    @torch.no_grad()
    def set_max_grad_norm(self, x):
        """None or <= 0: no clipping (the norm is still measured, a non-finite gradient still skips the update)."""
        self._need_grouped("set_max_grad_norm")
        self.max_grad_norm = None if x is None else float(x)
        self._ctrl[CTRL_MAX_NORM:CTRL_MAX_NORM + 1].copy_(torch.tensor([0.0 if x is None else float(x)], dtype=torch.float32))

    @torch.no_grad()
    def step(self, grad_scale=1.0, skip_word=None):
        """One update from the gradients currently in ``bucket.flat`` (pack them first).  ``skip_word``: a device int64
        tensor; the kernel leaves parameters and moments untouched when it is non-zero (engine.Trainer: the sticky error
        word of a timed-out stream wait).  A non-zero word is TERMINAL: it is sticky and the Trainer raises at its next
        step(), so the step counter below (which a skipped update still advances) never feeds another update.

        Grouped mode: squared norm, finish, Adam.  The device owns the step counter there and advances it only when the
        update is applied: a non-finite gradient (or a set ``skip_word``) leaves parameters, moments and the count as they
        were and adds one to ``skipped_updates``."""
        from ._native import check, lib
        dev = self.flat_p.device
        skip = skip_word.data_ptr() if skip_word is not None else None
        if self.grouped:
            n, S, G = self.flat_p.numel(), self._seg_group.numel(), len(self.param_groups)
            g = self.bucket.flat.data_ptr()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                tables = (self._seg_off.data_ptr(), self._seg_group.data_ptr(), S, G, self._seg_off_host.data_ptr(),
                          self._seg_group_host.data_ptr())
                check(lib.spacap_grad_sqnorm_f32(g, n, *tables, self._partials.data_ptr(), stream), "spacap_grad_sqnorm_f32")
                check(lib.spacap_optim_finish_f64(self._partials.data_ptr(), self._blocks, G, float(grad_scale), skip,
                                                  self.grad_sqnorm.data_ptr(), self._ctrl.data_ptr(), self._skipped.data_ptr(),
                                                  stream), "spacap_optim_finish_f64")
                check(lib.spacap_adam_flat_groups_f32(self.flat_p.data_ptr(), g, self.m.data_ptr(), self.v.data_ptr(), n, *tables,
                                                      self._hyper.data_ptr(), self.betas[0], self.betas[1], self.eps,
                                                      self._ctrl.data_ptr(), float(grad_scale), stream),
                      "spacap_adam_flat_groups_f32")
            return
        self.step_t += 1
        with torch.cuda.device(dev):
            check(lib.spacap_adam_flat_f32(self.flat_p.data_ptr(), self.bucket.flat.data_ptr(), self.m.data_ptr(),
                                           self.v.data_ptr(), self.flat_p.numel(), self.lr, self.betas[0], self.betas[1],
                                           self.eps, self.weight_decay, self.step_t.data_ptr(), float(grad_scale),
                                           skip, torch.cuda.current_stream(dev).cuda_stream), "spacap_adam_flat_f32")

    # -- torch-format state (both modes) ----------------------------------------------------------------------------------
    def _layout(self, param_groups):
        """The groups that number the state: this optimizer's own, or a caller's (engine.Trainer: the reference's two groups,
        also around an ungrouped optimizer) -- normalised and checked against the bucket either way."""
        if param_groups is None:
            groups = self.param_groups
            if not self.grouped:       # (one group; engine.Trainer.set_hyper writes .lr directly in this mode)
                groups = [dict(groups[0], lr=self.lr, weight_decay=self.weight_decay)]
            return groups
        return normalise_groups(self.bucket.params, param_groups, self.lr, self.weight_decay)[0]

    def state_dict(self, param_groups=None):
        """What ``torch.optim.Adam(param_groups).state_dict()`` holds after the same updates (reads the step count: a host
        synchronisation, for checkpoints only)."""
        groups = self._layout(param_groups)
        return pack_state_dict(groups, self.betas, self.eps, self.bucket.params, self.bucket.offsets, self.m, self.v,
                               int(float(self.step_t)))

    @torch.no_grad()
    def load_state_dict(self, sd, param_groups=None):
        """Moments, step count, ``lr`` and ``weight_decay`` from a ``torch.optim.Adam`` state dict of the same groups.  The
        state goes into the buffers a captured graph already reads: no re-capture."""
        groups = self._layout(param_groups)
        own = param_groups is None
        # (an ungrouped optimizer has ONE rate and ONE decay: refuse what it cannot represent before anything is written)
        hyper = [(float(a["lr"]), float(a["weight_decay"])) for a in sd["param_groups"]]
        if not self.grouped and len(set(hyper)) > 1:
            raise ValueError("FlatAdam: the loaded groups have different lr / weight_decay: build the optimizer with groups=")
        if self.grouped and not own:
            # the caller's groups must be this optimizer's own partition of the bucket, or the rates cannot be placed
            mine = [[id(p) for p in g["params"]] for g in self.param_groups]
            if [[id(p) for p in g["params"]] for g in groups] != mine:
                raise ValueError("FlatAdam.load_state_dict: param_groups differ from the optimizer's own groups")
        step, hyper = unpack_state_dict(sd, groups, self.bucket.params, self.bucket.offsets, self.m, self.v)
        self.step_t.fill_(float(step))
        if self.grouped:
            for g, (lr, wd) in zip(self.param_groups, hyper):
                g["lr"], g["weight_decay"] = lr, wd
            self.lr = hyper[0][0]
            self._write_hyper()
        else:
            self.lr, self.weight_decay = hyper[0]
