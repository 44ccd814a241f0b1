"""Multi-label diagnosis classification fine-tuning on the HIP engine: the reference's `MultimodalBertClf`
(Downstream_task/Classification/mmbt/models/mmbt.py: encoder -> tanh pooler -> Linear(H, n_classes)) with
`BCEWithLogitsLoss(pos_weight)` (mmbt/main.py:93-101) on top of a pretrained CXRBERT.

    model = CXRBertForClassification.from_pretrained(ckpt_dir, n_classes=14)          # main.py:241-242 (strict=False)
    out = model(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok)           # logits [B, C], differentiable
    loss = criterion(out, tgt); loss.backward(); optimizer.step()                     # main.py:213-217, verbatim
    loss = model(..., labels=tgt)                                                     # or: the fused loss + model.clf_stats
    probs = model.predict(...)                                                        # sigmoid probabilities under no_grad
    loss = model.fit_step(bank, idx, optimizer); out = model.evaluate(bank)           # from a data.ClassificationBank (DESIGN.md "8t")

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
    buffer (task.FlatHead).
    fit_step / evaluate: the same step, and the reference's model_eval with its per-class / macro / micro AUROC and F1, from a
    device-resident data.ClassificationBank -- the batch built by one HIP launch, the metrics from one launch of integer counts and one
    read-back per evaluation (DESIGN.md "8t")."""

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

    # ------------------------------------------------------------------ steps from a device-resident bank
    def _check_bank(self, bank):
        if bank.n_samples == 0 or bank.n_images == 0:
            raise ValueError("the bank is empty (ClassificationBank.add_samples, add_images)")
        if bank.n_classes != self.n_classes:
            raise ValueError(f"the bank holds targets over {bank.n_classes} classes, the classifier has {self.n_classes}")
        Lq = int(bank.img_feats.shape[1]) + int(bank.txt_ids.shape[1]) + 2
        if Lq > self.bert.cfg.max_pos:
            raise ValueError(f"the bank's sequences hold {Lq} positions ([CLS] + regions + [SEP] + text), max_position_embeddings is "
                             f"{self.bert.cfg.max_pos}")

    def fit_step(self, bank, idx, optimizer, mode="bi"):
        """One fine-tuning step (mmbt/main.py:208-217) from a data.ClassificationBank: optimizer.zero_grad(), the batch of the samples
        `idx` (one mv_clf_assemble launch), the loss node of forward(..., labels=target), its backward and optimizer.step().  mode:
        "s2s" / "bi" / "bar" or one per sample; "bi" is the reference's 1-D mask.  Returns the loss as a device scalar; clf_stats is
        updated as after forward.  Refused: several ranks, an empty bank, a bank over another class count, sequences longer than
        max_position_embeddings, a host idx outside the bank (IndexError)."""
        check_single_rank("CXRBertForClassification", "data-parallel fine-tuning is not supported (the head's gradients would not be "
                          "all-reduced); fine-tune on one rank, or run evaluate")
        self._check_bank(bank)
        with self._engine_state("training", "keep_acts"):
            optimizer.zero_grad()
            with torch.enable_grad():
                cls_tok, input_txt, desc, segment, img, sep_tok, target = bank.assemble(idx, mode=mode)
                loss = self(cls_tok, input_txt, desc, segment, img, sep_tok, labels=target)
                loss.backward()
        optimizer.step()
        return loss.detach()

    @torch.no_grad()
    def evaluate(self, bank, idx=None, batch_size=64, mode="bi"):
        """The reference's model_eval (mmbt/main.py:138-193) over the samples `idx` of a data.ClassificationBank (None: every sample, in
        order), in eval mode and without gradients; a last partial batch is allowed.  Every batch's sigmoid probabilities go into one
        [n, C] device buffer and its BCE sum into its slot of a per-batch buffer; one mv_clf_counts launch turns the probabilities and the
        bank's label bits into integer counts, and ONE read-back brings the counts and the loss bits over.  -> dict(loss (the mean of
        the batch means, main.py:145,158), auroc_per_class, macro_auroc, micro_auroc, macro_f1, micro_f1 (metrics_from_counters), n,
        counters int64 [C + 1, 7] on the host, probs f32 [n, C] on the device).  The engine's training / keep-activations /
        dropout-counter state is restored.  Pair counting is quadratic: n C <= 2^21 (beyond: metrics() on the host)."""
        if int(batch_size) < 1:
            raise ValueError("batch_size >= 1")
        self._check_bank(bank)
        eng = self.bert.engine
        # `take`: what the batches are cut from -- a host list stays a host list (its descriptors need no read-back)
        if torch.is_tensor(idx) and idx.device.type != "cpu":
            if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() == 0:
                raise TypeError("idx on the device: non-empty int32 [n]")
            dev_idx = take = idx.contiguous()
        else:
            take = bank.host_idx(torch.arange(bank.n_samples) if idx is None else idx)
            dev_idx = take.to(torch.int32).to(eng.device)
        n, C, bs = int(dev_idx.numel()), self.n_classes, int(batch_size)
        if n * C > ops.CLF_MAX_ELEMS:
            raise ValueError(f"evaluate: {n} samples x {C} classes is past the {ops.CLF_MAX_ELEMS} elements mv_clf_counts pairs up; "
                             "collect predict()'s probabilities and use classification.metrics() on the host")
        if not isinstance(mode, str) and len(mode) != n:
            raise ValueError(f"mode: one name, or one per sample ({n})")
        n_batches = (n + bs - 1) // bs
        probs = torch.empty((n, C), dtype=torch.float32, device=eng.device)
        sums = torch.zeros(n_batches, dtype=torch.float32, device=eng.device)
        with self._engine_state("training", "keep_acts", "drop_counter"):
            self._prepare(False)
            eng.training = False
            for k, s in enumerate(range(0, n, bs)):
                e = min(n, s + bs)
                cls_tok, input_txt, desc, segment, (feats, pos), sep_tok, target = bank.assemble(
                    take[s:e], mode=mode if isinstance(mode, str) else list(mode[s:e]))
                logits = self._encode_and_classify(cls_tok, input_txt, desc, segment, feats, pos, sep_tok)
                ops.bce_multilabel(logits, C, R=e - s, ld=self.Ap, target=target, pos_weight=self.pos_weight, loss=sums[k:k + 1],
                                   probs=probs[s:e])
            counters = ops.clf_counts(probs, dev_idx, bank.lab_bits, C)
        # the one read-back: the integer counters and the bits of the batches' f32 BCE sums
        host = torch.cat([counters.reshape(-1), sums.view(torch.int32).to(torch.int64)]).cpu()
        cnt = host[:counters.numel()].view(C + 1, ops.CLF_NCOUNT)
        bce = host[counters.numel():].to(torch.int32).view(torch.float32)
        sizes = torch.tensor([min(n, s + bs) - s for s in range(0, n, bs)], dtype=torch.float32) * float(C)
        out = metrics_from_counters(cnt)
        out.update(loss=float((bce / sizes).double().mean()), n=n, counters=cnt, probs=probs)
        return out

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
    macro_f1, micro_f1 = _f1(cnt[0], cnt[1], cnt[2])
    return dict(auroc_per_class=per, macro_auroc=sum(per) / C, micro_auroc=_auroc(p.reshape(-1), t.reshape(-1)),
                macro_f1=macro_f1, micro_f1=micro_f1)


def _f1(tp, fp, fn):
    """(macro, micro) F1 from f64 [C] counts; a zero denominator scores 0."""
    den = 2 * tp + fp + fn
    f1 = torch.where(den > 0, 2 * tp / den.clamp(min=1), torch.zeros_like(den))
    mden = float(2 * tp.sum() + fp.sum() + fn.sum())
    return float(f1.mean()), (float(2 * tp.sum()) / mden if mden > 0 else 0.0)


def metrics_from_counters(counters):
    """mv_clf_counts' integer counters [C + 1, 7] = {n_pos, n_neg, gt, eq, tp, fp, fn} (rows 0 .. C-1 one class each, row C all n C
    elements as one list) -> what `metrics` returns, formed from exact integers: AUROC = (2 gt + eq) / (2 n_pos n_neg) -- the
    tie-averaged rank statistic of _auroc, bit for bit -- or 0 when a label value is missing (main.py:167-171); macro AUROC the mean
    with those zeros; F1 from the class rows at the reference's threshold, zero on a zero denominator."""
    c = torch.as_tensor(counters).detach().cpu().to(torch.int64)
    if c.dim() != 2 or c.shape[1] != 7 or c.shape[0] < 2:
        raise ValueError("metrics_from_counters: counters [C + 1, 7]")
    C = int(c.shape[0]) - 1
    rows = c.tolist()

    def auroc(r):
        n_pos, n_neg, gt, eq = r[:4]
        return (2 * gt + eq) / (2 * n_pos * n_neg) if n_pos and n_neg else 0.0

    per = [auroc(r) for r in rows[:C]]
    cls = c[:C].double()
    macro_f1, micro_f1 = _f1(cls[:, 4], cls[:, 5], cls[:, 6])
    return dict(auroc_per_class=per, macro_auroc=sum(per) / C, micro_auroc=auroc(rows[C]), macro_f1=macro_f1, micro_f1=micro_f1)
