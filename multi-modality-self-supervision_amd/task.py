"""What the fine-tuning models share (DESIGN.md "8i"): `TaskModel`, a CXRBERT plus the engine-state handling of one task forward, and
`FlatHead`, a TaskModel whose few head Parameters are views of one padded flat fp32 buffer with 16-bit copies (the VQA answer
classifier, the diagnosis classifier).  The backward of every task's autograd node goes through cxrbert.run_backward."""
from __future__ import annotations

import weakref
from contextlib import contextmanager
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import hip_ops as ops
from ._lib import MV_F16, MV_F32
from .cxrbert import CXRBERT


def check_single_rank(who, why):
    """Fine-tuning is single-rank: nothing all-reduces a task's gradients.  Refused where a gradient is wanted under several ranks."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError(f"{who}: {why}")


class TaskModel(nn.Module):
    """.bert is the CXRBERT; `_unreached` names the encoder tensors the task's graph never reaches (`grad is None` in the reference:
    medvill_amd.optim.BertAdam neither updates nor decays them)."""

    _unreached = ()

    def __init__(self, config, args=None, **kw):
        super().__init__()
        self.bert = CXRBERT(config, args, **kw)

    def _prepare(self, want_grad):
        bert = self.bert
        eng = bert.engine
        # Parameters stepped by an outside optimizer (or loaded): refresh the 16-bit copies -- unless medvill_amd.optim's kernels, which
        # write them, were the last to touch them (version counters, as CXRBERT's forward)
        if not bert.__dict__.pop("_shadow_fresh", False):
            eng.shadow_dirty = eng.shadow_dirty or bert._params_dirty()
        eng.training = bool(self.training)       # dropout only in train mode
        eng.keep_acts = bool(want_grad)          # under torch.no_grad() nothing is saved for a backward

    def _pack(self, attn_mask):
        """Mask descriptors whose padding is invisible, on a 16-bit path: the encoder runs on the valid rows only."""
        from .data import MaskDesc
        return isinstance(attn_mask, MaskDesc) and self.bert.engine.is16 and attn_mask.packable()

    def encode_cls_rows(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok):
        """The encoder with its last layer's per-row work on the B [CLS] rows only (Engine.encoder_forward, empty tail_rows)."""
        eng = self.bert.engine
        none = torch.arange(int(input_txt.shape[0]), device=eng.device, dtype=torch.int32)[:0]
        return eng.encoder_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, pack=self._pack(attn_mask), tail_rows=none)

    @contextmanager
    def _engine_state(self, *fields):
        """The engine's state is sticky: a later direct Engine user must find the named fields as they were."""
        eng = self.bert.engine
        prev = [getattr(eng, f) for f in fields]
        try:
            yield eng
        finally:
            for f, v in zip(fields, prev):
                setattr(eng, f, v)


class FlatHead(TaskModel):
    """A task head of a few Parameters stored as views of `head_p`, one flat fp32 buffer laid out by `_layout` (name -> (offset, shape),
    `_n_head` elements; the weight named `_padded_key` owns `Ap` rows, the rows past its shape staying zero).  head_sh / head_shf: the
    16-bit copies the kernels read, in the encodings the engine uses; head_g, head_m / head_v: gradient and optimizer moments, allocated
    when first needed.  A subclass declares `_head_keys` / `_padded_key`, builds the modules those names point into, calls `_init_head`
    and defines `reset_head`."""

    _head_keys = ()
    _padded_key = None

    def _init_head(self, layout):
        eng = self.bert.engine
        self._layout, self._n_head, self.Ap = layout
        dev = eng.device
        self.head_p = torch.zeros(self._n_head, dtype=torch.float32, device=dev)
        self.head_g = self.head_m = self.head_v = None
        # 16-bit copies in the encodings the engine uses (the same rule as Engine.shadow / shadow_f)
        self.head_sh = torch.zeros(self._n_head, dtype=torch.bfloat16, device=dev) if eng.shadow is not None else None
        self.head_shf = torch.zeros(self._n_head, dtype=torch.float16, device=dev) if eng.shadow_f is not None else None
        self._hplist = []
        for name in self._head_keys:
            mod, leaf = name.rsplit(".", 1)
            par = nn.Parameter(self._view(self.head_p, name), requires_grad=True)
            par._medvill_head = weakref.ref(self)          # medvill_amd.optim finds the head's flat buffers through it
            self.get_submodule(mod)._parameters[leaf] = par
            self._hplist.append(par)
        self._head_versions = None
        self.reset_head()

    # ------------------------------------------------------------------ storage
    def _view(self, buf, name, padded=False):
        off, shape = self._layout[name]
        if padded and name == self._padded_key:
            shape = (self.Ap, shape[1])
        n = 1
        for s in shape:
            n *= s
        return buf[off:off + n].view(shape)

    def _shadow_of(self, dt):
        return self.head_p if dt == MV_F32 else (self.head_shf if dt == MV_F16 else self.head_sh)

    def _rebind(self):
        for name, par in zip(self._head_keys, self._hplist):
            par.data = self._view(self.head_p, name)
        if self.head_g is not None:
            for name, par in zip(self._head_keys, self._hplist):
                if par.grad is not None and par.grad.device != self.head_g.device:
                    par.grad = None

    def _apply(self, fn, *a, **k):
        # .to(device) / .cuda(): the encoder moves its flat buffers (CXRBERT._apply), the head its own; the Parameters stay views
        self.bert._apply(fn, *a, **k)
        dev = self.bert.engine.device
        for k_ in ("head_p", "head_g", "head_m", "head_v", "head_sh", "head_shf"):
            t = getattr(self, k_)
            if t is not None:
                setattr(self, k_, t.to(dev))
        self._head_versions = None
        self._rebind()
        return self

    def _head_dirty(self):
        v = self._head_versions
        return v is None or v != sum(p._version for p in self._hplist)

    def _head_written(self):
        """The 16-bit copies match the fp32 master as of now (version counters, as CXRBERT._params_dirty)."""
        self._head_versions = sum(p._version for p in self._hplist)

    def _sync_head(self):
        """16-bit copies of the head from its fp32 master (after an outside optimizer or a load changed the Parameters)."""
        for sh in (self.head_sh, self.head_shf):
            if sh is not None:
                ops.cast(self.head_p, sh, self._n_head)
        self._head_written()

    def _prepare(self, want_grad):
        super()._prepare(want_grad)
        if self.bert.engine.is16 and self._head_dirty():
            self._sync_head()

    # ------------------------------------------------------------------ gradients
    def _zero_head_grad(self):
        if self.head_g is None:
            self.head_g = torch.zeros_like(self.head_p)
        else:
            self.head_g.zero_()

    def _head_holds_views(self):
        return any(p.grad is not None and p.grad.data_ptr() == self._view(self.head_g, n).data_ptr() for n, p in zip(self._head_keys, self._hplist))

    def _hand_over_head(self, views):
        """The head's gradients -> torch, by the rule of cxrbert._hand_over_grads (views of the flat gradient unless a hook or a
        process group asks for copies)."""
        out = []
        for name, p in zip(self._head_keys, self._hplist):
            g = self._view(self.head_g, name)
            if views and (p.grad is None or p.grad.data_ptr() == g.data_ptr()):
                p.grad = g
                out.append(None)
            else:
                out.append(g.clone())
        return tuple(out)

    def _gather_head_grads(self):
        """Before an optimizer's launch over the head: every .grad that is not the view of head_g already is copied into it, and the
        moment buffers exist."""
        if self.head_g is None:
            self.head_g = torch.zeros_like(self.head_p)
        for name, p in zip(self._head_keys, self._hplist):
            gv = self._view(self.head_g, name)
            if p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad)
        if self.head_m is None:
            self.head_m, self.head_v = torch.zeros_like(self.head_p), torch.zeros_like(self.head_p)

    # ------------------------------------------------------------------ state dict
    def _head_state(self, out):
        for name, p in zip(self._head_keys, self._hplist):
            out[name] = p.detach().clone()
        return out

    def _load_state(self, head, rest, strict):
        """`rest` into the encoder (its MLM / ITM heads may be absent: the task models have neither), `head` (the head's entries of the
        state dict) into the flat buffer -- or, when the dict holds none (a pretraining checkpoint), reset_head()."""
        r = self.bert.load_state_dict(rest, strict=False)
        missing = [k_ for k_ in r.missing_keys if not k_.startswith(("mlm.", "itm."))]
        unexpected = list(r.unexpected_keys) + [k_ for k_ in head if k_ not in self._head_keys]
        with torch.no_grad():
            if head:
                for name in self._head_keys:
                    if name in head:
                        self._view(self.head_p, name).copy_(head[name].to(self.head_p.device, torch.float32))
                    else:
                        missing.append(name)
            else:
                self.reset_head()
        self._head_versions = None
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)
