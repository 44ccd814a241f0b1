"""The optimizer line of the reference's trainer on the engine's flat buffers.

The reference builds `AdamW(self.model.parameters(), lr=args.lr)` from transformers.optimization (train_origin.py:15, 60) and calls
`optimizer.zero_grad(); loss.backward(); optimizer.step()` (train_origin.py:129-131).  `medvill_amd.optim.AdamW` is that class for a
medvill_amd.CXRBERT: the same constructor arguments and update rule (HF AdamW: eps outside the square root, decoupled weight decay,
`correct_bias`), one fused kernel over the flat fp32 master / moment buffers that also writes the 16-bit weight copies the MFMA kernels read
-- so the next forward has nothing to convert (a torch optimizer on the Parameters makes every forward refresh 110 M weights).

    from medvill_amd.optim import AdamW
    self.optimizer = AdamW(self.model.parameters(), lr=args.lr)          # train_origin.py:60, unchanged otherwise

It follows torch.optim.Optimizer's protocol (param_groups for schedulers, zero_grad, state_dict / load_state_dict) with ONE parameter group: the
update runs over the whole flat buffer, so per-group hyper-parameters and partial parameter sets are refused.
"""
from __future__ import annotations

import torch


class _FlatState:
    """state_dict / load_state_dict of an optimizer over the engine's flat buffers (`_model`) and, when the Parameters of a task head
    were passed with them, over that head's (`_task`, a task.FlatHead): the step count `_t`, the groups' hyper-parameters and the
    moment buffers (flat_m / flat_v, head_m / head_v) on the host."""

    def state_dict(self):
        eng = self._model.engine
        eng.wait_optimizer()
        eng.ensure_opt()
        sd = {"step": self._t, "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
              "flat_m": eng.flat_m.detach().cpu(), "flat_v": eng.flat_v.detach().cpu()}
        task = self._task
        if task is not None and task.head_m is not None:
            sd["head_m"], sd["head_v"] = task.head_m.detach().cpu(), task.head_v.detach().cpu()
        return sd

    def load_state_dict(self, sd):
        eng = self._model.engine
        eng.wait_optimizer()
        eng.ensure_opt()
        if tuple(sd["flat_m"].shape) != tuple(eng.flat_m.shape):
            raise ValueError("optimizer state of a different model configuration")
        eng.flat_m.copy_(sd["flat_m"].to(eng.device))
        eng.flat_v.copy_(sd["flat_v"].to(eng.device))
        task = self._task
        if task is not None and "head_m" in sd:
            if tuple(sd["head_m"].shape) != tuple(task.head_p.shape):
                raise ValueError("optimizer state of a different task head")
            task.head_m, task.head_v = sd["head_m"].to(task.head_p.device).clone(), sd["head_v"].to(task.head_p.device).clone()
        self._t = int(sd["step"])
        for g, s in zip(self.param_groups, sd.get("param_groups", [])):
            g.update({k: v for k, v in s.items() if k != "params"})


class AdamW(_FlatState, torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, overlap=False):
        """overlap=True: the update runs per parameter range on the engine's side stream and the next forward waits range by range (what the
        fused training step does: the HBM-bound update hides under the next step's first layers).  Anything ELSE that reads the Parameters on
        the current stream right after step() must then call `model.engine.wait_optimizer()` first -- hence opt-in."""
        params = list(params)
        if not params or isinstance(params[0], dict):
            raise ValueError("medvill_amd.optim.AdamW takes model.parameters() of ONE medvill_amd.CXRBERT (a single parameter group)")
        ref = getattr(params[0], "_medvill_model", None)
        model = ref() if ref is not None else None
        if model is None:
            raise ValueError("these are not the Parameters of a medvill_amd.CXRBERT: use a torch optimizer")
        own = {id(p) for p in model._plist}
        extra = [p for p in params if id(p) not in own]
        # a task model's parameters (task.FlatHead): the encoder's flat buffer plus the task head's own flat buffer (one more fused
        # launch per step).  Only the head of THIS encoder, and all of it; any other foreign parameter is refused below
        task = _task_of(model, extra)
        head_ids = {id(q) for q in task._hplist} if task is not None else set()
        head = [p for p in extra if id(p) in head_ids]
        if head and len({id(p) for p in head}) != len(head_ids):
            raise ValueError("medvill_amd.optim.AdamW updates the task head's whole flat buffer: pass ALL of its parameters")
        extra = [p for p in extra if id(p) not in head_ids]
        if len({id(p) for p in params} & own) != len(own):
            raise ValueError("medvill_amd.optim.AdamW updates the model's whole flat parameter buffer: pass ALL of model.parameters() "
                             "(freeze by other means, or use a torch optimizer for a subset)")
        if extra and any(p.requires_grad for p in extra):
            # e.g. a trainable region encoder: not in the flat buffer
            raise ValueError(f"{len(extra)} parameters do not belong to the CXRBERT's flat buffer (a trainable image encoder?): give those to a "
                             "torch optimizer of their own")
        super().__init__([p for p in params if id(p) in own] + head,
                         dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self._model, self._t, self.overlap = model, 0, bool(overlap)
        self._task = task if head else None

    @torch.no_grad()
    def step(self, closure=None):
        from . import hip_ops as ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model, task = self._model, self._task
        eng = model.engine
        grads = [p.grad for p in model._plist]
        if all(g is None for g in grads):
            return loss                                   # nothing was back-propagated since zero_grad(): like torch, no update
        if any(g is None for g in grads):
            raise RuntimeError("some Parameters have a gradient and some have none: the flat update cannot skip individual tensors")
        eng.ensure_grad()
        for n, g in zip(model._param_names, grads):       # normally every .grad IS the view of the flat buffer (CXRBERT.grad_views)
            if g.data_ptr() != eng.g[n].data_ptr():
                eng.g[n].copy_(g)
        hp = self.param_groups[0]
        self._t += 1
        eng.adamw_step(self._t, lr=float(hp["lr"]), betas=tuple(hp["betas"]), eps=float(hp["eps"]), weight_decay=float(hp["weight_decay"]),
                       correct_bias=bool(hp["correct_bias"]), overlap=self.overlap)
        hgrads = [p.grad for p in task._hplist] if task is not None else []
        if any(g is None for g in hgrads) and not all(g is None for g in hgrads):
            raise RuntimeError("some classifier Parameters have a gradient and some have none: the flat update cannot skip individual tensors")
        if hgrads and hgrads[0] is not None:        # the task head: same hyper-parameters, same step count
            task._gather_head_grads()
            ops.adamw_step(task.head_p, task.head_g, task.head_m, task.head_v, task.head_sh, task._n_head, float(hp["lr"]), hp["betas"][0],
                           hp["betas"][1], float(hp["eps"]), float(hp["weight_decay"]), self._t, bool(hp["correct_bias"]), 1.0,
                           shadow_f16=task.head_shf)
            task._head_written()             # the kernel has written the 16-bit copies too
        # the kernel has written the 16-bit copies: until somebody else modifies a Parameter in place (version counters), forwards need not
        model._opt_versions = sum(p._version for p in model._plist)
        return loss


def _task_of(model, extra):
    """The task model (task.FlatHead: CXRBertForVQA, CXRBertForClassification) whose encoder is `model` and whose head Parameters,
    marked with `_medvill_head`, are among `extra` (None otherwise)."""
    for p in extra:
        ref = getattr(p, "_medvill_head", None)
        task = ref() if ref is not None else None
        if task is not None and task.bert is model:
            return task
    return None


# ======================================================================================================================== BertAdam
_NO_CHANGE = ("params", "weight_decay")


def schedule_factor(schedule: str, x: float, warmup: float) -> float:
    """The reference's SCHEDULES (optimization.py:33-55) in Python floats; the kernel evaluates the same expressions in double."""
    import math
    if x < warmup:
        return x / warmup
    if schedule == "warmup_constant":
        return 1.0
    if schedule == "warmup_cosine":
        return 0.5 * (1.0 + math.cos(math.pi * x))
    if schedule == "warmup_linear":
        return max((x - 1.0) / (warmup - 1.0), 0)
    raise ValueError(f"Invalid schedule parameter: {schedule}")


def build_tables(entries, chunk=None):
    """entries: (offset, count, decay, active) per tensor, in buffer order -> (tensors int64 [T, 4], chunks int32 [NC]) on the host, the
    tables of mv_tensor_sqnorms / mv_bertadam_step: row t = {offset, count, first_chunk, decay | active << 1}; tensor t owns
    ceil(count / chunk) consecutive chunk slots.  Offsets must be 64-element aligned and the ranges disjoint (the gaps between them
    belong to no chunk: the kernels never touch them)."""
    from .hip_ops import OPTIM_CHUNK
    chunk = OPTIM_CHUNK if chunk is None else int(chunk)
    rows, ids, end = [], [], 0
    for t, (off, cnt, decay, active) in enumerate(entries):
        off, cnt = int(off), int(cnt)
        if off % 64 or cnt <= 0 or off < end:
            raise ValueError(f"tensor {t}: offset {off} (64-aligned, ascending, disjoint) count {cnt}")
        end = off + cnt
        rows.append([off, cnt, len(ids), (1 if decay else 0) | (2 if active else 0)])
        ids.extend([t] * ((cnt + chunk - 1) // chunk))
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4), torch.tensor(ids, dtype=torch.int32)


class _Tables:
    """Device tables + norm workspace of one flat buffer."""

    def __init__(self, entries, device):
        self.tensors_host, self.chunks_host = build_tables(entries)
        self.tensors, self.chunks = self.tensors_host.to(device), self.chunks_host.to(device)
        self.partials = torch.zeros(self.chunks.numel(), dtype=torch.float32, device=device)
        self.sq = torch.zeros(self.tensors.shape[0], dtype=torch.float32, device=device)


class BertAdam(_FlatState, torch.optim.Optimizer):
    """The reference's fine-tuning optimizer (pytorch_pretrained_bert/optimization.py:57-182) on the flat buffers: per TENSOR gradient-norm
    clipping, weight decay on the tensors of the groups that ask for it, a warm-up schedule evaluated on `step` BEFORE its increment (so
    the first step under warm-up moves nothing but updates the moments) and no bias correction.  Two launches per flat buffer
    (mv_tensor_sqnorms, mv_bertadam_step); the second also writes the 16-bit weight copies.

        optimizer = BertAdam(optimizer_grouped_parameters, lr=args.lr, warmup=args.warmup, t_total=t_total)      # main.py:115-126

    `params`: model.parameters() or the reference's grouped list; groups may differ in `weight_decay` only, and the positive values
    must agree (the kernel takes one value and a per-tensor flag).  Ownership as AdamW: all Parameters of ONE CXRBERT, optionally plus
    the whole head of its CXRBertForVQA / CXRBertForClassification, or the CXRBERT of a CXRBertForReportFinetune (no head Parameters).
    Tensors the task's graph does not reach (named by the task module: MLM / ITM heads, the pooler under VQA; the ITM head and the
    pooler under report fine-tuning) are `grad is None` in the reference and stay bit-unchanged here.  Differences, documented:
    one step counter for all tensors (the reference keeps one per tensor; they only diverge for a tensor that has a gradient in some
    steps and none in others, which is refused here), and `.grad` is left unclipped."""

    def __init__(self, params, lr, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01,
                 max_grad_norm=1.0):
        from .hip_ops import SCHEDULE_IDS
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if schedule not in SCHEDULE_IDS:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        if t_total != -1 and t_total <= 0:
            raise ValueError("Invalid t_total: {} - should be positive or -1".format(t_total))
        groups = list(params)
        if not groups:
            raise ValueError("medvill_amd.optim.BertAdam got an empty parameter list")
        if not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        groups = [dict(g, params=list(g["params"])) for g in groups]
        flat = [p for g in groups for p in g["params"]]
        ref = next((getattr(p, "_medvill_model", None) for p in flat if getattr(p, "_medvill_model", None) is not None), None)
        model = ref() if ref is not None else None
        if model is None:
            raise ValueError("these are not the Parameters of a medvill_amd.CXRBERT: use a torch optimizer")
        if len({id(p) for p in flat}) != len(flat):
            raise ValueError("a Parameter appears in more than one group")
        own = {id(p) for p in model._plist}
        extra = [p for p in flat if id(p) not in own]
        task = _task_of(model, extra)
        head_ids = {id(q) for q in task._hplist} if task is not None else set()
        n_head = sum(1 for p in extra if id(p) in head_ids)
        if n_head and n_head != len(head_ids):
            raise ValueError("medvill_amd.optim.BertAdam updates the task head's whole flat buffer: pass ALL of its parameters")
        extra = [p for p in extra if id(p) not in head_ids]
        if len({id(p) for p in flat} & own) != len(own):
            raise ValueError("medvill_amd.optim.BertAdam updates the model's whole flat parameter buffer: pass ALL of model.parameters() "
                             "(freeze by other means, or use a torch optimizer for a subset)")
        if extra:
            raise ValueError(f"{len(extra)} parameters belong neither to the CXRBERT's flat buffer nor to its task head (a trainable "
                             "image encoder?): give those to a torch optimizer of their own")
        super().__init__(groups, dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e,
                                      weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            diff = [k for k in g0 if k not in _NO_CHANGE and g.get(k) != g0[k]]
            if diff:
                raise ValueError(f"parameter groups may differ in weight_decay only (the update is one launch per flat buffer): {diff}")
        if len({float(g["weight_decay"]) for g in self.param_groups if g["weight_decay"] > 0.0}) > 1:
            raise ValueError("parameter groups with different positive weight_decay values: the kernel takes one value and a per-tensor flag")
        self._model, self._task, self._t = model, (task if n_head else None), 0
        # a task module without head Parameters (CXRBertForReportFinetune) registers itself on its encoder: it contributes the names of
        # the tensors its graph does not reach, nothing else.  A bare CXRBERT carries no such reference
        ref = getattr(model, "_headless_task", None)
        self._headless = ref() if (ref is not None and self._task is None) else None
        self._tab = self._htab = self._ent = None
        self._decay_key = None

    # ------------------------------------------------------------------ tables
    def _decay_ids(self):
        return {id(p) for g in self.param_groups if g["weight_decay"] > 0.0 for p in g["params"]}

    def _refresh(self):
        """The per-tensor entries (and the device tables made from them) are cached; they depend on which groups decay, so a change of
        a group's weight_decay between zero and positive (param_groups, load_state_dict) rebuilds them."""
        key = tuple(g["weight_decay"] > 0.0 for g in self.param_groups)
        if key != self._decay_key:
            self._decay_key, self._ent, self._tab, self._htab = key, None, None, None

    def _entries(self):
        """(offset, count, decay, active) per tensor of the encoder's flat buffer, in layout order: one entry per Parameter of the
        reference's named_parameters() -- query, key and value separately although adjacent; the tied decoder matrix is the word
        embedding, once -- with the tensors the task does not reach marked inactive."""
        self._refresh()
        if self._ent is not None:
            return self._ent
        model = self._model
        decay = self._decay_ids()
        # (the task module is known through its head's Parameters: an encoder passed alone is updated whole)
        off_graph = tuple(getattr(self._task if self._task is not None else self._headless, "_unreached", ()))
        out = []
        for name, par in zip(model._param_names, model._plist):
            off, shape = model.engine.layout[name]
            out.append((off, par.numel(), id(par) in decay, not name.startswith(off_graph) if off_graph else True))
        self._ent = out
        return out

    def _head_entries(self):
        task = self._task
        decay = self._decay_ids()
        return [(task._layout[name][0], par.numel(), id(par) in decay, True) for name, par in zip(task._head_keys, task._hplist)]

    def _tables(self):
        self._refresh()
        dev = self._model.engine.device
        if self._tab is None or self._tab.tensors.device != dev:
            self._tab = _Tables(self._entries(), dev)
            self._htab = _Tables(self._head_entries(), dev) if self._task is not None else None
        return self._tab, self._htab

    # ------------------------------------------------------------------ torch.optim protocol
    def _hyper(self):
        g0 = self.param_groups[0]
        if any(g["lr"] != g0["lr"] for g in self.param_groups[1:]):
            raise RuntimeError("the learning rates of the parameter groups have diverged: one launch per flat buffer takes one lr")
        pos = {float(g["weight_decay"]) for g in self.param_groups if g["weight_decay"] > 0.0}
        if len(pos) > 1:
            raise RuntimeError("parameter groups now hold different positive weight_decay values: the kernel takes one value and a flag")
        return g0, (pos.pop() if pos else 0.0)

    def get_lr(self):
        """optimization.py:96-110: the scheduled learning rate per updated Parameter at the current step count; [0] before the first step."""
        if self._t == 0:
            return [0]
        g, _ = self._hyper()
        lr = g["lr"] * schedule_factor(g["schedule"], self._t / g["t_total"], g["warmup"]) if g["t_total"] != -1 else g["lr"]
        tab = self._entries()
        return [lr] * (sum(1 for e_ in tab if e_[3]) + (len(self._task._hplist) if self._task is not None else 0))

    @torch.no_grad()
    def step(self, closure=None):
        from . import hip_ops as ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model, task = self._model, self._task
        eng = model.engine
        entries = self._entries()
        active = [e_[3] for e_ in entries]
        grads = [p.grad for p in model._plist]
        hgrads = [p.grad for p in task._hplist] if task is not None else []
        need = [g for g, a in zip(grads, active) if a] + hgrads
        if all(g is None for g in need):
            return loss                                   # nothing was back-propagated since zero_grad(): like the reference, no update
        if any(g is None for g in need):
            raise RuntimeError("some Parameters have a gradient and some have none: this optimizer keeps ONE step count, so a tensor "
                               "cannot sit a step out (tensors the task never reaches are skipped by the task module's table)")
        hp, wd = self._hyper()
        tab, htab = self._tables()
        eng.ensure_opt()
        eng.wait_optimizer()
        for n, g, a in zip(model._param_names, grads, active):       # normally every .grad IS the view of the flat buffer
            if a and g.data_ptr() != eng.g[n].data_ptr():
                eng.g[n].copy_(g)
        # (no scaler_state: like optim.AdamW, gradients arrive already checked -- the autograd nodes redo an overflowed backward)
        kw = dict(lr=float(hp["lr"]), step=self._t, warmup=float(hp["warmup"]), t_total=int(hp["t_total"]), schedule=hp["schedule"],
                  b1=float(hp["b1"]), b2=float(hp["b2"]), eps=float(hp["e"]), weight_decay=wd, max_grad_norm=float(hp["max_grad_norm"]))
        clip = kw["max_grad_norm"] > 0
        if clip:
            ops.tensor_sqnorms(eng.flat_g, tab.tensors, tab.chunks, tab.partials, tab.sq)
        ops.bertadam_step(eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, tab.tensors, tab.chunks, tab.sq if clip else None,
                          shadow=eng.shadow, shadow_f16=eng.shadow_f, **kw)
        eng.shadow_dirty = False
        eng.refresh_w2t()
        if task is not None:
            task._gather_head_grads()
            if clip:
                ops.tensor_sqnorms(task.head_g, htab.tensors, htab.chunks, htab.partials, htab.sq)
            ops.bertadam_step(task.head_p, task.head_g, task.head_m, task.head_v, htab.tensors, htab.chunks, htab.sq if clip else None,
                              shadow=task.head_sh, shadow_f16=task.head_shf, **kw)
            task._head_written()             # the kernel has written the 16-bit copies too
        self._t += 1
        # the kernel has written the 16-bit copies: until somebody else modifies a Parameter in place (version counters), forwards need not
        model._opt_versions = sum(p._version for p in model._plist)
        return loss
