"""Mirror of the reference's retrieval head (Downstream_task/Retrieval/retrieval.py:12-32): ITM-style matching on
top of CXRBERT.enc + .itm with 1-D attention masks (the `attn_mask.dim() == 2` branch, cxrbert_origin.py:76-77).
Encoder-only inference / fine-tuning through the same HIP kernels."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip_ops as ops
from .checkpoint import hf_config, write_pretrained
from .cxrbert import CXRBERT, run_backward
from .task import TaskModel, check_single_rank

_SINGLE_RANK = ("CXRBertForRetrieval", "data-parallel fine-tuning through forward(labels=) / fit_step is not supported (single "
                "rank, as classification); fine-tune on one rank, or run evaluation under torch.no_grad()")


# ---------------------------------------------------------------------------------------------------- host side of evaluate()
def group_plan(n_pairs: int, group_size: int, batch_size: int):
    """An evaluation file of G groups of `group_size` candidates, in batches: -> (G, [(start, stop), ...]).  The reference reshapes its
    flat result list with np.reshape(..., [-1, eval_len_size]) (full_dset_retrieval.py:257-259), which needs a whole number of groups."""
    n_pairs, group_size, batch_size = int(n_pairs), int(group_size), int(batch_size)
    if group_size < 1 or batch_size < 1:
        raise ValueError("group_size and batch_size must be positive")
    if n_pairs < 1 or n_pairs % group_size != 0:
        raise ValueError(f"{n_pairs} pairs do not form whole groups of {group_size} candidates")
    return n_pairs // group_size, [(s, min(s + batch_size, n_pairs)) for s in range(0, n_pairs, batch_size)]


def summarize(counters, ks):
    """mv_rank_groups' integer counters (include/medvill.h) -> the reference's numbers: dict(hits, recall, precision: {"R@k": value},
    mrr_score, groups, groups_without_aligned).  Recall is the mean over the groups that hold an aligned candidate (the reference
    divides by zero on the others); the reference rounds recall and precision to 3 decimals where it builds its dictionaries (:309-313),
    the values here are unrounded."""
    c = [int(v) for v in counters]
    G, none = c[0], c[1]
    fx = float(2 ** 32)
    hits, rec, prec = {}, {}, {}
    for q, k in enumerate(ks):
        name = f"R@{int(k)}"
        hits[name] = c[4 + q] / G
        rec[name] = (c[12 + q] / fx) / (G - none) if G > none else float("nan")
        prec[name] = c[20 + q] / (int(k) * G)
    return dict(hits=hits, recall=rec, precision=prec, mrr_score=(c[2] / fx) / G, groups=G, groups_without_aligned=none)


def aligned_list(pos, labels, group_size, ids=None):
    """compute_ranks' Aligned_lst (:261-269): per group [id of the best-placed aligned candidate, rank]; a group without an aligned
    candidate lists its LAST candidate in the order with rank = group_size, as the reference's loop leaves it.  pos, labels: host
    integer arrays [G * C]; ids: the candidates' ids (default: their position in the flat list)."""
    import numpy as np
    C = int(group_size)
    pos, lab = np.asarray(pos).reshape(-1, C), np.asarray(labels).reshape(-1, C)
    idv = (np.arange(pos.size) if ids is None else np.asarray(ids)).reshape(-1, C)
    out = []
    for g in range(pos.shape[0]):
        al = np.flatnonzero(lab[g] == 1)
        if al.size:
            j = int(al[np.argmin(pos[g][al])])
            out.append([int(idv[g, j]), int(pos[g, j])])
        else:
            out.append([int(idv[g, int(np.argmax(pos[g]))]), C])
    return out


class _RetLossFn(torch.autograd.Function):
    """Encoder (last layer on the [CLS] rows) + pooler + ITM head + mean cross-entropy as one autograd node: the retrieval counterpart
    of classification._ClfFn (train(), full_dset_retrieval.py:367-379, without the logits' hand-over and torch's loss kernels)."""

    @staticmethod
    def forward(ctx, model, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, labels, *params):
        ctx.model, ctx.B, ctx.labels = model, int(input_txt.shape[0]), labels
        loss, ctx.logits = model._loss_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, labels)
        return loss

    @staticmethod
    def backward(ctx, g):
        model = ctx.model
        return (None,) * 9 + run_backward(model.bert, lambda: model._loss_backward(ctx.logits, ctx.labels, ctx.B, g))


class CXRBertForRetrieval(TaskModel):
    def __init__(self, config, args=None, **kw):
        super().__init__(config, args, **kw)
        self.enc, self.itm = self.bert.enc, self.bert.itm

    @classmethod
    def from_pretrained(cls, path, args=None, **kw):
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.bert = CXRBERT.from_pretrained(path, args=args, **kw)
        m.enc, m.itm = m.bert.enc, m.bert.itm
        return m

    def forward(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, labels=None):
        """-> ITM logits [B,2] (retrieval.py:26-31: `_, cls, _ = self.enc(...); return self.itm(cls)` -- that literal form works
        too, `enc` and `itm` are callable; this is the same arithmetic as ONE autograd node, without the hand-over tensors).
        labels [B] (1 = aligned; not part of the reference's signature): -> the mean cross-entropy over the rows, differentiable, as one
        node (_RetLossFn); `model.stats` f32 [3] on the device += [nll_sum, rows, correct] (reset_stats() clears) -- the running loss
        and accuracy of train() (:382-391) without a read-back per step."""
        if labels is None:
            return self.bert._itm_only(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok)
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError
        bert = self.bert
        eng = bert.engine
        B = int(input_txt.shape[0])
        lab = torch.as_tensor(labels).to(eng.device, torch.int32).reshape(-1).contiguous()
        if lab.numel() != B:
            raise ValueError(f"labels must hold one entry per row ({B}), got {lab.numel()}")
        feats, pos = bert._regions(input_img)
        self._want_grad = torch.is_grad_enabled()
        if self._want_grad:
            check_single_rank(*_SINGLE_RANK)
        return _RetLossFn.apply(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, lab, *bert._plist)

    # ------------------------------------------------------------------ fused loss
    def reset_stats(self):
        self.stats = torch.zeros(3, dtype=torch.float32, device=self.bert.engine.device)

    def _logits_cls_rows(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok):
        """Encoder (packed where the mask allows it; last layer's per-row work on the B [CLS] rows only) + pooler + ITM head ->
        the engine's f32 [B, 2] logit buffer."""
        self.encode_cls_rows(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
        return self.bert.engine._itm_forward()

    def _loss_forward(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, labels):
        eng = self.bert.engine
        B = int(input_txt.shape[0])
        self._prepare(getattr(self, "_want_grad", True))       # (set by forward / fit_step; the engine state stays as this call set it)
        logits = self._logits_cls_rows(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
        st = torch.zeros(3, dtype=torch.float32, device=eng.device)
        ops.ce_fwd_bwd(logits, 2, labels, B, 2, st)
        if getattr(self, "stats", None) is None or self.stats.device != st.device:
            self.reset_stats()
        self.stats += st
        return st[0] / float(B), logits

    def _loss_backward(self, logits, labels, B, g):
        """d(mean CE) into the flat gradient: mv_ce_fwd_bwd under the device loss scale, ITM head, pooler, encoder."""
        eng = self.bert.engine
        H = self.bert.cfg.hidden
        eng.zero_grad()
        d8 = eng._buf("ditm8", (B, 8), eng.adt)
        gs = g.detach().to(eng.device, torch.float32).reshape(1) / float(B)          # d(mean) = upstream / B, on the device
        scratch = eng._buf("ret_ce_scratch", (3,), torch.float32)
        scratch.zero_()
        ops.ce_fwd_bwd(logits, 2, labels, B, 2, scratch, d8, 8, grad_scale_dev=gs, loss_scale_dev=eng.loss_scale_dev)
        eng.dhidden_buffer()                                              # the compact final state's gradient: the pooler path fills it
        eng._itm_backward(d8)
        eng.encoder_backward()

    def fit_step(self, bank, idx, lr, step, key=0, draws=None, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0):
        """One fine-tuning step of train() (:357-380) from a RetrievalBank: the sampler's negatives for the positives `idx` (dataset
        indices, image i and text i being a pair), the 2B pair batch, the loss, its backward and the engine's fused AdamW -- HF AdamW's
        defaults, which the reference's `AdamW(model.parameters(), lr=args.lr)` has.  step = 1, 2, ... (bias correction; with `key` it also
        selects the sampler's random words; `draws` overrides them, see hip_ops.pair_negatives).  f16 gradients: an overflowed step is
        skipped and the loss scale backs off on the device, as in TrainStep.  Returns the step's mean loss as a device scalar; nothing
        is read back except the 2B mask descriptors (the packed-row plan needs the row count on the host)."""
        check_single_rank(*_SINGLE_RANK)
        eng = self.bert.engine
        n = bank.n_texts
        if n != bank.n_images or n < 2:
            raise ValueError("fit_step: the bank must hold n >= 2 items with image i and text i forming a pair")
        idx = torch.as_tensor(idx)
        if idx.device.type == "cpu" and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"fit_step: idx outside the data set of {n} items")
        idx = idx.to(eng.device, torch.int32).reshape(-1).contiguous()
        pairs, labels = ops.pair_negatives(idx, n, key=key, step=step, class_id=bank.class_id, draws=draws)
        cls_tok, input_txt, desc, segment, (feats, pos), sep_tok = bank.assemble(pairs)
        eng.ensure_opt()
        self._want_grad = True
        with torch.no_grad():
            loss, logits = self._loss_forward(cls_tok, input_txt, desc, segment, feats, pos, sep_tok, labels)
            self._loss_backward(logits, labels, int(labels.numel()), torch.ones(1, device=eng.device))
            eng.check_overflow()
            eng.adamw_step(int(step), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, use_scaler=True)
        self.bert._opt_versions = sum(p._version for p in self.bert._plist)      # the kernel refreshed the 16-bit copies as well
        return loss

    @torch.no_grad()
    def evaluate(self, bank, pairs, labels, group_size, ks=(1, 5, 10), batch_size=100, ids=None):
        """test() + evaluate() of the reference (:461-510, :326-339) from a RetrievalBank: the ITM logits of all pairs, batch by batch,
        into one device buffer; one mv_rank_groups launch; ONE read-back at the end.  pairs [G * group_size, 2] (image item, text
        item), group after group; labels [G * group_size] (1 = aligned).  Eval mode, no gradients; the engine's training /
        keep-activations / dropout-counter state is restored.  -> dict(hits, recall, precision: {"R@k": value}, mrr_score,
        Aligned_lst: [[candidate, rank], ...] (candidate = ids[...] when given, else the position in `pairs`), eval_loss: the mean of
        the batches' mean cross-entropy (:502), groups, groups_without_aligned, p f32 [G*C] / pos int32 [G*C] / rank int32 [G]:
        device tensors (include/medvill.h, mv_rank_groups, for the order among ties))."""
        eng = self.bert.engine
        dev = eng.device
        n_pairs = len(pairs)
        G, plan = group_plan(n_pairs, group_size, batch_size)
        ks = tuple(int(k) for k in ks)
        if len(ks) > 8 or any(k < 1 for k in ks):
            raise ValueError("ks: at most 8 positive cut-offs")
        on_dev = torch.is_tensor(pairs) and pairs.device.type != "cpu"
        if not on_dev:
            from .data import check_pairs
            pairs = check_pairs(pairs, bank.n_images, bank.n_texts)
        lab = torch.as_tensor(labels).reshape(-1)
        if lab.numel() != n_pairs:
            raise ValueError(f"labels must hold one entry per pair ({n_pairs}), got {lab.numel()}")
        lab = lab.to(dev, torch.int32).contiguous()
        logits_all = torch.empty((n_pairs, 2), dtype=torch.float32, device=dev)
        ce = torch.zeros((len(plan), 3), dtype=torch.float32, device=dev)
        eng.shadow_dirty = eng.shadow_dirty or self.bert._params_dirty()
        with self._engine_state("training", "keep_acts", "drop_counter"):      # (the dropout counter too: a run of evaluation forwards)
            eng.training, eng.keep_acts = False, False
            for b, (s, e) in enumerate(plan):
                cls_tok, input_txt, desc, segment, (feats, pos), sep_tok = bank.assemble(pairs[s:e])
                logits = self._logits_cls_rows(cls_tok, input_txt, desc, segment, feats, pos, sep_tok)
                logits_all[s:e].copy_(logits)
                ops.ce_fwd_bwd(logits, 2, lab[s:e], e - s, 2, ce[b])
        p, pos_, rank, counters = ops.rank_groups(logits_all, lab, group_size, ks)
        # the one read-back: counters | per-batch loss sums (f32 bit patterns) | pos | labels
        host = torch.cat([counters, ce[:, 0].contiguous().view(torch.int32).to(torch.int64), pos_.to(torch.int64), lab.to(torch.int64)]).cpu()
        nb = len(plan)
        out = summarize(host[:ops.RANK_NCOUNT].tolist(), ks)
        sums = host[ops.RANK_NCOUNT:ops.RANK_NCOUNT + nb].to(torch.int32).view(torch.float32)
        out["eval_loss"] = float(sum(float(sums[b]) / (e - s) for b, (s, e) in enumerate(plan)) / nb)
        o = ops.RANK_NCOUNT + nb
        out["Aligned_lst"] = aligned_list(host[o:o + n_pairs].numpy(), host[o + n_pairs:].numpy(), group_size, ids=ids)
        out["p"], out["pos"], out["rank"] = p, pos_, rank
        return out

    def save_pretrained(self, save_directory):
        """config.json + pytorch_model.bin under the reference model's key names (its modules are `enc` and `itm`,
        Downstream_task/Retrieval/retrieval.py:24-25); from_pretrained -- here and CXRBERT's -- loads it back."""
        sd = {k: v for k, v in self.bert.state_dict().items() if k.startswith(("enc.", "itm."))}
        write_pretrained(save_directory, hf_config(self.bert.cfg, "CXRBertForRetrieval"), sd)

    @torch.no_grad()
    def score(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok):
        """P(aligned) per pair, as full_dset_retrieval.py:461-510 ranks candidates.  When `attn_mask` is a
        `data.MaskDesc` of a family whose padding is invisible (the retrieval scripts' 1-D masks are), the encoder runs
        on the valid rows only (inference form of the padding removal)."""
        if self._pack(attn_mask):
            feats, pos = self.bert._regions(input_img)
            with self._engine_state("training", "keep_acts") as eng:
                eng.training, eng.keep_acts = False, False
                eng.encoder_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, pack=True)
                logits = eng._itm_forward().clone()
        else:
            logits = self.forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok)
        return torch.softmax(logits.float(), dim=-1)[:, 1]


class CXRBertForGeneration(nn.Module):
    """Report generation from a pretrained CXRBERT (the reference's BertForSeq2SeqDecoder use of it, driven by generation_decode.py):
    a thin holder whose `generate` is CXRBERT.generate (KV-cached greedy / beam search on the HIP kernels)."""

    def __init__(self, config, args=None, **kw):
        super().__init__()
        self.bert = CXRBERT(config, args, **kw)

    @classmethod
    def from_pretrained(cls, path, args=None, **kw):
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.bert = CXRBERT.from_pretrained(path, args=args, **kw)
        return m

    def generate(self, cls_tok, input_img, sep_tok, **kw):
        return self.bert.generate(cls_tok, input_img, sep_tok, **kw)

    def evaluate(self, bank, idx=None, batch_size=64, **generate_kwargs):
        """Corpus BLEU-1..4 of the reports generated for the items of a data.ReportBank: report_eval.evaluate (DESIGN.md "8u")."""
        from .report_eval import evaluate
        return evaluate(self, bank, idx=idx, batch_size=batch_size, **generate_kwargs)

    forward = generate
