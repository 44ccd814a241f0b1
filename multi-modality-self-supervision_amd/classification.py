"""Multi-label diagnosis classification fine-tuning on the HIP engine: the reference's `MultimodalBertClf`
(Downstream_task/Classification/mmbt/models/mmbt.py: encoder -> tanh pooler -> Linear(H, n_classes)) with
`BCEWithLogitsLoss(pos_weight)` (mmbt/main.py:93-101) on top of a pretrained CXRBERT.

    model = CXRBertForClassification.from_pretrained(ckpt_dir, n_classes=14)          # main.py:241-242 (strict=False)
    out = model(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok)           # logits [B, C], differentiable
    loss = criterion(out, tgt); loss.backward(); optimizer.step()                     # main.py:213-217, verbatim
    loss = model(..., labels=tgt)                                                     # or: the fused loss + model.clf_stats
    probs = model.predict(...)                                                        # sigmoid probabilities under no_grad

The encoder runs its last layer's per-row work on the B [CLS] rows only (Engine.encoder_forward, tail_rows=[]), as VQA training; the
engine's pooler feeds `clf`; unlike VQA the pooler gets a gradient (Engine._pooler_backward), the ITM and MLM heads get none.  `clf`
lives in a small flat buffer of its own with C padded to a multiple of 16 (padding rows stay zero): task.FlatHead, as the VQA head.
Arithmetic is CXRBERT's (the pretrained model), DESIGN.md "8c".
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from . import hip_ops as ops
from ._lib import EPI_BIAS
from .checkpoint import hf_config, read_pretrained, write_pretrained
from .cxrbert import run_backward
from .task import FlatHead, check_single_rank
from .vqa import _ROWS

CLF_KEYS = ("clf.weight", "clf.bias")


def clf_layout(H: int, C: int):
    """name -> (offset, shape) of the head's flat buffer, its size and the padded class count Cp (C rounded up to 16)."""
    Cp = (C + 15) // 16 * 16
    lay, off = OrderedDict(), 0
    for name, shape, n in ((CLF_KEYS[0], (C, H), Cp * H), (CLF_KEYS[1], (C,), Cp)):
        lay[name] = (off, shape)
        off += (n + 63) // 64 * 64
    return lay, off, Cp


class _ClfFn(torch.autograd.Function):
    """Encoder + pooler + clf (+ BCE) as one autograd node.  mode "loss": -> mean BCEWithLogits(pos_weight); "logits": -> [B, C]."""

    @staticmethod
    def forward(ctx, model, mode, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, target, *params):
        eng = model.bert.engine
        B, C = int(input_txt.shape[0]), model.n_classes
        logits = model._encode_and_classify(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
        ctx.model, ctx.mode, ctx.B, ctx.logits, ctx.target = model, mode, B, logits, target
        if mode == "logits":
            return logits[:, :C].clone()
        loss = torch.zeros(1, dtype=torch.float32, device=eng.device)
        if model.clf_stats is None:
            model.reset_stats()
        ops.bce_multilabel(logits, C, R=B, ld=model.Ap, target=target, pos_weight=model.pos_weight, loss=loss, counters=model.clf_stats)
        return loss[0] / float(B * C)

    @staticmethod
    def backward(ctx, g):
        model = ctx.model
        return (None,) * 10 + run_backward(model.bert, lambda: model._backward_once(ctx, g), head=model)


class CXRBertForClassification(FlatHead):
    """forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, labels=None):
         labels None -> differentiable f32 logits [B, C];  labels [B, C] multi-hot float -> the mean BCEWithLogitsLoss (with
         `pos_weight` when set), and `model.clf_stats` f32 [3, C] on the device += {tp, fp, fn} at threshold 0.5 (reset_stats() clears).
    .bert is the CXRBERT (its pooler is the head's first half), .clf the Linear(H, C) whose Parameters are views of the head's flat
    buffer (task.FlatHead)."""

    _head_keys = CLF_KEYS
    _padded_key = CLF_KEYS[0]
    _unreached = ("mlm.", "itm.")            # medvill_amd.optim.BertAdam: no update, no decay (the pooler IS reached here)

    def __init__(self, config, args=None, n_classes=14, pos_weight=None, task_type="multilabel", **kw):
        if task_type != "multilabel":
            raise NotImplementedError(f"task_type={task_type!r}: only the multi-label task (the reference's default) is built")
        super().__init__(config, args, **kw)
        H, C = self.bert.cfg.hidden, int(n_classes)
        if C <= 0:
            raise ValueError("n_classes must be positive")
        self.n_classes = C
        self.clf = nn.Linear(H, C)
        self.clf_stats = None
        self._init_head(clf_layout(H, C))
        self.pos_weight = None
        if pos_weight is not None:
            self.set_pos_weight(pos_weight)

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        dev = self.bert.engine.device
        for k_ in ("pos_weight", "clf_stats"):
            t = getattr(self, k_, None)
            if t is not None:
                setattr(self, k_, t.to(dev))
        return self

    @torch.no_grad()
    def reset_head(self, seed: int | None = None):
        """nn.Linear's default init (the reference builds `clf` as a plain nn.Linear), seeded from torch.initial_seed() unless given."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(torch.initial_seed() if seed is None else seed)
        H, C = self.bert.cfg.hidden, self.n_classes
        bound = 1.0 / (H ** 0.5)
        flat = torch.zeros(self._n_head, dtype=torch.float32)
        self._view(flat, CLF_KEYS[0]).copy_((torch.rand((C, H), generator=gen) * 2 - 1) * bound)
        self._view(flat, CLF_KEYS[1]).copy_((torch.rand((C,), generator=gen) * 2 - 1) * bound)
        self.head_p.copy_(flat.to(self.head_p.device))
        self._head_versions = None

    def set_pos_weight(self, pos_weight):
        """f32 [C] positive-class weights of BCEWithLogitsLoss (get_criterion, main.py:93-101); None removes them."""
        if pos_weight is None:
            self.pos_weight = None
            return
        w = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1).to(self.bert.engine.device).contiguous()
        if w.numel() != self.n_classes:
            raise ValueError(f"pos_weight must hold {self.n_classes} entries, got {w.numel()}")
        self.pos_weight = w

    def reset_stats(self):
        self.clf_stats = torch.zeros(3, self.n_classes, dtype=torch.float32, device=self.bert.engine.device)

    # ------------------------------------------------------------------ forward / backward
    def _encode_and_classify(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok):
        """Encoder (last layer on the B [CLS] rows) + the engine's pooler + clf -> logits [B, Cp] f32 (columns C..Cp-1 unspecified)."""
        eng = self.bert.engine
        B = int(input_txt.shape[0])
        H, C, Cp = self.bert.cfg.hidden, self.n_classes, self.Ap
        self.encode_cls_rows(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
        pooled = eng.S["pooled_f"]
        W = self._view(self._shadow_of(eng.fdt), CLF_KEYS[0], padded=True)
        b = self._view(self.head_p, CLF_KEYS[1])
        logits = eng._buf("clf_logits", (B, Cp), torch.float32)
        if eng.is16:
            for r0 in range(0, B, _ROWS):
                m = min(_ROWS, B - r0)
                ops.gemm_rows(pooled[r0:r0 + m], W, logits[r0:r0 + m], M=m, N=C, K=H, ldc=Cp, bias=b, epi=EPI_BIAS)
        else:
            ops.gemm(pooled, W, logits, M=B, N=C, K=H, ldc=Cp, bias=b, epi=EPI_BIAS)
        return logits

    def _backward_once(self, ctx, g):
        eng = self.bert.engine
        B, C, Cp, H = ctx.B, self.n_classes, self.Ap, self.bert.cfg.hidden
        eng.zero_grad()
        self._zero_head_grad()
        adt, us = eng.adt, eng.unscale_dev
        dl = eng._buf("clf_dlogits", (B, Cp), adt)
        if ctx.mode == "loss":
            gs = g.detach().to(eng.device, torch.float32).reshape(1) / float(B * C)      # d(mean) = upstream / (B * C), on the device
            ops.bce_multilabel(ctx.logits, C, R=B, ld=Cp, target=ctx.target, pos_weight=self.pos_weight, dgrad=dl, ldd=Cp,
                               grad_scale_dev=gs, loss_scale_dev=eng.loss_scale_dev)
        else:
            d32 = g.detach().to(eng.device, torch.float32).contiguous()
            ls = eng.loss_scale_dev
            dl.zero_()
            ops.cast2d(d32 if ls is None else d32 * ls, C, dl, Cp, B, C)
        # clf: db, dW = dl^T . pooled, dpooled = dl . W (contraction over the padded Cp columns: the padding of dl is zero)
        ops.colsum(dl, Cp, B, C, self._view(self.head_g, CLF_KEYS[1]), accumulate=True, unscale=us)
        eng._dW(dl, eng.S["pooled"], self._view(self.head_g, CLF_KEYS[0]), C, H, B, lda=Cp, ldb=H)
        dpool = eng._buf("dpool", (B, H), adt)
        ops.gemm(dl, self._view(self._shadow_of(eng.dt), CLF_KEYS[0], padded=True), dpool, tb=True, M=B, N=H, K=Cp, lda=Cp, ldb=H)
        eng.dhidden_buffer()                                           # the compact final state's gradient: the pooler path fills it
        eng._pooler_backward(dpool)                                    # tanh backward, pooler gradients, dh[CLS]
        eng.encoder_backward()

    def forward(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, labels=None):
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError
        feats, pos = self.bert._regions(input_img)
        want_grad = torch.is_grad_enabled()
        if want_grad:
            check_single_rank("CXRBertForClassification", "data-parallel fine-tuning is not supported (the head's gradients would not be "
                              "all-reduced); fine-tune on one rank, or run inference under torch.no_grad()")
        eng = self.bert.engine
        B, C = int(input_txt.shape[0]), self.n_classes
        target = None
        if labels is not None:
            target = torch.as_tensor(labels).to(eng.device, torch.float32).contiguous()
            if tuple(target.shape) != (B, C):
                raise ValueError(f"labels must be the multi-hot [B, C] = [{B}, {C}], got {tuple(target.shape)}")
        self._prepare(want_grad)                 # (engine state NOT restored after the call, as VQA; the report model restores it)
        params = list(self.bert._plist) + self._hplist
        return _ClfFn.apply(self, "logits" if target is None else "loss", cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok,
                            target, *params)

    @torch.no_grad()
    def predict(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok):
        """sigmoid probabilities f32 [B, C]."""
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError
        feats, pos = self.bert._regions(input_img)
        with self._engine_state("training", "keep_acts") as eng:
            self._prepare(False)
            logits = self._encode_and_classify(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
            probs = torch.empty(int(input_txt.shape[0]), self.n_classes, dtype=torch.float32, device=eng.device)
            ops.bce_multilabel(logits, self.n_classes, ld=self.Ap, probs=probs)
        return probs

    # ------------------------------------------------------------------ state dict (MultimodalBertClf's layout)
    def state_dict(self, *a, **k):
        """CXRBERT's enc.* names (aliases included) plus clf.weight / clf.bias -- no mlm.* / itm.* (the model has neither head)."""
        out = OrderedDict((k_, v) for k_, v in self.bert.state_dict().items() if k_.startswith("enc."))
        return self._head_state(out)

    def load_state_dict(self, sd, strict=True):
        """This layout, or a CXRBERT pretraining state dict (enc.* / mlm.* / itm.*: the head then starts from reset_head()).  The
        reference's unused enc.clf.* and its enc.img_encoder.* are ignored."""
        head = {k_: v for k_, v in sd.items() if k_ in CLF_KEYS}
        rest = OrderedDict((k_, v) for k_, v in sd.items() if k_ not in CLF_KEYS and not k_.startswith(("enc.clf.", "enc.img_encoder.")))
        return self._load_state(head, rest, strict)

    def save_pretrained(self, save_directory):
        write_pretrained(save_directory, hf_config(self.bert.cfg, "CXRBertForClassification", n_classes=self.n_classes), self.state_dict())

    @classmethod
    def from_pretrained(cls, path_or_state_dict, config=None, args=None, n_classes=None, **kw):
        config, sd = read_pretrained(path_or_state_dict, config)
        if n_classes is None:
            w = sd.get(CLF_KEYS[0])
            n_classes = int(w.shape[0]) if w is not None else int(config.get("n_classes", 14) if isinstance(config, dict) else 14)
        m = cls(config, args, n_classes=n_classes, **kw)
        m.load_state_dict(sd, strict=False)
        return m


# ---------------------------------------------------------------------------------------------------- metrics (torch, no sklearn)
def _auroc(score, y):
    """Rank statistic (Mann-Whitney U / (n+ n-)); ties get the average rank; a class with one label value scores 0 (main.py:167-171)."""
    y = y > 0.5
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        return 0.0
    s = score.double()
    order = torch.argsort(s)
    ss = s[order]
    uniq, inv, cnt = torch.unique_consecutive(ss, return_inverse=True, return_counts=True)
    end = torch.cumsum(cnt, 0).double()
    ranks = (end - (cnt.double() - 1) / 2.0)[inv]           # average 1-based rank of each tie group
    r = torch.empty_like(ranks)
    r[order] = ranks
    return float((r[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def metrics(probs, targets, counters=None):
    """probs, targets [N, C] -> dict(auroc_per_class [C], macro_auroc, micro_auroc, macro_f1, micro_f1).  F1 at threshold 0.5 from
    the device counters f32 [3, C] {tp, fp, fn} when given (model.clf_stats), else counted from probs > 0.5."""
    p, t = torch.as_tensor(probs).detach().float().cpu(), torch.as_tensor(targets).detach().float().cpu()
    C = p.shape[1]
    per = [_auroc(p[:, c], t[:, c]) for c in range(C)]
    if counters is None:
        pred, pos = p > 0.5, t > 0.5
        cnt = torch.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)]).double()
    else:
        cnt = torch.as_tensor(counters).detach().double().cpu().reshape(3, C)
    tp, fp, fn = cnt[0], cnt[1], cnt[2]
    den = 2 * tp + fp + fn
    f1 = torch.where(den > 0, 2 * tp / den.clamp(min=1), torch.zeros_like(den))
    mden = float(2 * tp.sum() + fp.sum() + fn.sum())
    return dict(auroc_per_class=per, macro_auroc=sum(per) / C, micro_auroc=_auroc(p.reshape(-1), t.reshape(-1)),
                macro_f1=float(f1.mean()), micro_f1=(float(2 * tp.sum()) / mden if mden > 0 else 0.0))
