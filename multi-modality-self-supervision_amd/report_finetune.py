"""Report-generation fine-tuning on the HIP engine: the reference's `BertForPreTrainingLossMask(tasks='report_generation')`
(Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:903-1054, finetune.py:430-469) on top of a pretrained
CXRBERT -- the model that produces the weights `CXRBERT.generate` / `CXRBertForGeneration` decode.

    model = CXRBertForReportFinetune.from_pretrained(ckpt_dir, label_smoothing=0.1)      # finetune.py:338-351
    loss, _ = model(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok,
                    masked_lm_labels=ids, masked_pos=pos, masked_weights=w, drop_worst_ratio=0.0)
    loss.backward(); optimizer.step()                                                    # finetune.py:443-451

The objective (model.py:998-1005,1043-1054; loss.py:12-48): the predictions are LISTED -- position, label and weight per slot, padded
to max_pred with (0, 0, 0), a position possibly listed twice -- the per-slot loss is a KL divergence against a label-smoothed target
(or plain cross-entropy, label 0 included, without smoothing), the int(B (1 - drop_worst_ratio)) samples with the smallest weighted
loss sums are kept and the result is normalised by their weight sum + 1e-5.  Here the list becomes a plan over the DISTINCT consumed
rows (`build_plan`): the encoder's last layer, the transform and the tied decoder run on those U rows only (Engine.encoder_forward,
tail_rows), and the objective and its gradient are the three kernels of csrc/mv_lmloss.hip.  The pooler and the ITM / sequence
relationship head never reach the loss: their gradients are zero and medvill_amd.optim.BertAdam leaves them untouched, like the
reference's `grad is None`.  DESIGN.md "8e. Report fine-tuning".
"""
from __future__ import annotations

import weakref
from types import SimpleNamespace

import torch

from . import hip_ops as ops
from . import report_eval
from .checkpoint import from_finetune_keys, hf_config, read_pretrained, to_finetune_keys, write_pretrained
from .cxrbert import run_backward
from .task import TaskModel, check_single_rank


def keep_count(B: int, drop_worst_ratio: float) -> int:
    """The number of samples loss_mask_and_normalize keeps: the reference's own Python expression (model.py:1002)."""
    return int(B * (1 - drop_worst_ratio))


def build_plan(masked_pos, masked_lm_labels, masked_weights, L: int, V: int, valid_len=None) -> dict:
    """Host plan of one batch: (pos, ids, w) [B, max_pred] -> the distinct consumed rows and the prediction entries in CSR form over them.
      rows int32 [U]      flat logical positions b * L + pos, ascending (the encoder's tail_rows)
      row_ptr int32 [U+1] entries of row u: row_ptr[u] .. row_ptr[u+1]-1, in slot order
      labels int32 [n], weights f32 [n], sample int32 [n]
    Zero-weight slots are dropped first (the reference's value and gradients do not depend on them: that is its padding).  A position
    listed twice keeps both entries, with equal or different labels.  Refused: position 0 (a labelled row is never a sample's first
    row: that row belongs to the pooler), a position outside the sequence or -- valid_len int [B], packed rows -- past the sample's
    valid length, a label outside [0, V), a negative or non-finite weight."""
    pos = torch.as_tensor(masked_pos).detach().cpu().to(torch.int64)
    ids = torch.as_tensor(masked_lm_labels).detach().cpu().to(torch.int64)
    w = torch.as_tensor(masked_weights).detach().cpu().to(torch.float32)
    if pos.dim() != 2 or pos.shape != ids.shape or pos.shape != w.shape:
        raise ValueError(f"masked_pos, masked_lm_labels and masked_weights must share one [B, max_pred] shape, got {tuple(pos.shape)}, "
                         f"{tuple(ids.shape)}, {tuple(w.shape)}")
    B = int(pos.shape[0])
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("masked_weights must be finite and >= 0")
    on = w > 0
    b_idx = torch.arange(B, dtype=torch.int64).view(B, 1).expand_as(pos)[on]
    p, t, wt = pos[on], ids[on], w[on]
    if bool((p == 0).any()):
        raise ValueError("masked_pos lists position 0 ([CLS]) with a non-zero weight: the report model predicts text positions only")
    if bool(((p < 0) | (p >= L)).any()):
        raise ValueError(f"masked_pos outside the sequence (0 < position < {L})")
    if valid_len is not None:
        vl = torch.as_tensor(valid_len).detach().cpu().to(torch.int64).view(-1)
        if bool((p >= vl[b_idx]).any()):
            raise ValueError("masked_pos lists a position past the sample's valid length (after the text [SEP]): packed rows hold no "
                             "such row.  Pass the materialised mask to run every row")
    if bool(((t < 0) | (t >= V)).any()):
        raise ValueError(f"masked_lm_labels outside the vocabulary [0, {V})")
    flat = b_idx * L + p
    rows, inv = torch.unique(flat, sorted=True, return_inverse=True)
    order = torch.argsort(inv, stable=True)                 # entries grouped by row, slot order kept inside a row
    U = int(rows.numel())
    row_ptr = torch.zeros(U + 1, dtype=torch.int64)
    if U:
        row_ptr[1:] = torch.cumsum(torch.bincount(inv, minlength=U), 0)
    return dict(B=B, U=U, n=int(order.numel()), rows=rows.to(torch.int32), row_ptr=row_ptr.to(torch.int32),
                labels=t[order].to(torch.int32).contiguous(), weights=wt[order].contiguous(), sample=b_idx[order].to(torch.int32).contiguous())


class _ReportFn(torch.autograd.Function):
    """Encoder (last layer on the distinct consumed rows) + MLM head + the objective as one autograd node."""

    @staticmethod
    def forward(ctx, model, plan, k, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, *params):
        ctx.model, ctx.plan = model, plan
        ctx.saved = model._forward_loss(plan, k, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
        return model.lm_stats[0].clone()

    @staticmethod
    def backward(ctx, g):
        model = ctx.model
        return (None,) * 10 + run_backward(model.bert, lambda: model._backward_once(ctx, g))


class CXRBertForReportFinetune(TaskModel):
    """`BertForPreTrainingLossMask(config, args, tasks='report_generation')` with this package's CXRBERT input convention:
        forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, masked_lm_labels=, masked_pos=, masked_weights=,
                drop_worst_ratio=0.0) -> (masked_lm_loss, dummy zero [1])                               (model.py:1054)
    masked_pos / masked_lm_labels / masked_weights [B, max_pred]: positions index the full sequence [CLS] + N regions + [SEP] + text
    (data_loader.py:353-419); host tensors (what a DataLoader hands over) are planned on the host, device tensors cost one read-back.
    model.lm_stats: f32 [4] on the device = [loss, kept weight sum, kept sample count, kept entries whose argmax is the label].
    `attn_mask`: a materialised 2-D / 3-D mask or data.MaskDesc (16-bit paths: the encoder then runs on the valid rows only).
    .bert is the CXRBERT; there are no head Parameters.  `label_smoothing` as config.label_smoothing of the reference (0: plain CE).
    fit_step / eval_step: the same objective from a device-resident data.ReportBank -- batch, masking draw and row plan built by HIP
    kernels, one read-back per step (DESIGN.md "8q")."""

    # medvill_amd.optim.BertAdam: the encoder tensors this task's graph never reaches (`grad is None` in the reference)
    _unreached = ("itm.", "enc.pooler.")

    def __init__(self, config, args=None, label_smoothing=None, **kw):
        super().__init__(config, args, **kw)
        if label_smoothing is None:
            label_smoothing = (config.get("label_smoothing") if isinstance(config, dict) else getattr(config, "label_smoothing", None)) or 0.0
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError("label_smoothing must lie in [0, 1] (loss.py:20)")
        if label_smoothing > 0.0 and self.bert.cfg.vocab_size < 3:
            raise ValueError("label smoothing spreads its mass over V - 2 columns: V >= 3")
        self.label_smoothing = label_smoothing
        self.lm_stats = self.lm_keep = None
        # a task without head Parameters: medvill_amd.optim.BertAdam finds it (and _unreached) through the encoder
        self.bert._headless_task = weakref.ref(self)

    # ------------------------------------------------------------------ forward
    def _forward_loss(self, plan, k, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok):
        eng = self.bert.engine
        dev = eng.device
        B, U = plan["B"], plan["U"]
        pack = self._pack(attn_mask)
        # (a host plan -- build_plan's -- is uploaded here; a device plan -- mv_report_plan's, fit_step / eval_step -- stays where it is)
        d = {k_: plan[k_].to(dev) for k_ in ("rows", "row_ptr", "labels", "weights", "sample")}
        eng.encoder_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, pack=pack, tail_rows=d["rows"])
        S, V = eng.S, self.bert.cfg.vocab_size
        if U > 0:
            logits = eng._mlm_forward(S["hidden_f"][:U], S["hidden"][:U], U, "rf_")
            Vp = int(logits.shape[1])
            loss_e, hit, row_stat = ops.lm_loss_fwd(logits, d["row_ptr"], d["labels"], self.label_smoothing, U=U, V=V, ld=Vp)
        else:                                    # every weight is zero: the reference's loss is 0 / 1e-5
            logits, Vp, row_stat = None, 0, None
            loss_e = torch.zeros(0, dtype=torch.float32, device=dev)
            hit = torch.zeros(0, dtype=torch.int32, device=dev)
        keep, stats, inv = ops.lm_loss_select(loss_e, d["weights"], d["sample"], hit, B, k)
        self.lm_stats, self.lm_keep = stats, keep
        return dict(d=d, logits=logits, Vp=Vp, row_stat=row_stat, keep=keep, inv=inv, S=S)

    def _backward_once(self, ctx, g):
        eng = self.bert.engine
        sv, plan = ctx.saved, ctx.plan
        B, U, H, V = plan["B"], plan["U"], self.bert.cfg.hidden, self.bert.cfg.vocab_size
        eng.S = sv["S"]
        eng.zero_grad()
        if U == 0:
            return                               # nothing weighted: every gradient is zero
        d = sv["d"]
        gd = g.detach().to(eng.device, torch.float32).reshape(1)
        dl = torch.empty((U, sv["Vp"]), dtype=eng.adt, device=eng.device)
        ops.lm_loss_bwd(sv["logits"], d["row_ptr"], d["labels"], d["weights"], d["sample"], self.label_smoothing, sv["row_stat"],
                        sv["keep"], sv["inv"], gd, dl, U=U, V=V, ld=sv["Vp"], ldd=sv["Vp"], loss_scale_dev=eng.loss_scale_dev)
        dxr = eng._mlm_backward(dl, "rf_")
        dhid = eng.dhidden_buffer()
        dhid[:U].copy_(dxr)
        dhid[U:].zero_()                         # the B first rows: the pooler / ITM / sequence-relationship heads receive nothing
        eng.encoder_backward()

    def forward(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, masked_lm_labels=None, masked_pos=None,
                masked_weights=None, drop_worst_ratio=0.0):
        if masked_lm_labels is None or masked_pos is None or masked_weights is None:
            raise ValueError("CXRBertForReportFinetune.forward needs masked_lm_labels, masked_pos and masked_weights (model.py:1043-1053); "
                             "decode with CXRBertForGeneration / CXRBERT.generate")
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError            # model.py:952-957
        feats, pos = self.bert._regions(input_img)
        want_grad = torch.is_grad_enabled()
        if want_grad:
            check_single_rank("CXRBertForReportFinetune", "data-parallel fine-tuning is not supported (drop-worst selects over the whole "
                              "batch and the gradients would not be all-reduced); fine-tune on one rank, or evaluate under torch.no_grad()")
        B, N = int(input_txt.shape[0]), int(feats.shape[1])
        Lq = N + int(input_txt.shape[1]) + 2
        trio = (masked_pos, masked_lm_labels, masked_weights)
        if all(torch.is_tensor(t) and t.is_cuda for t in trio) and len({tuple(t.shape) for t in trio}) == 1:
            host = torch.stack([t.to(torch.float64) for t in trio]).cpu()      # one read-back of the three small arrays
            trio = (host[0].to(torch.int64), host[1].to(torch.int64), host[2].to(torch.float32))
        pack = self._pack(attn_mask)
        plan = build_plan(*trio, L=Lq, V=self.bert.cfg.vocab_size, valid_len=attn_mask.host_desc()[:, 2] if pack else None)
        if plan["B"] != B:
            raise ValueError(f"masked_pos holds {plan['B']} samples, the batch {B}")
        k = keep_count(B, drop_worst_ratio)
        if not 0 <= k <= B:
            raise ValueError(f"drop_worst_ratio {drop_worst_ratio} keeps {k} of {B} samples")
        with self._engine_state("training", "keep_acts"):       # restored after the call (the VQA / classification forwards leave it set)
            self._prepare(want_grad)
            loss = _ReportFn.apply(self, plan, k, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, *self.bert._plist)
        return loss, loss.new_zeros(1)           # (masked_lm_loss, dummy_value), model.py:1054

    # ------------------------------------------------------------------ steps from a device-resident bank
    def _bank_loss(self, bank, idx, step, key, mode, drop_worst_ratio, draws):
        """data.ReportBank.assemble -> mv_report_plan -> the _ReportFn node on the device plan (the caller has set the engine state).
        ONE read-back: the plan's counts {U, n, bad} -- the engine sizes its launches with U on the host."""
        cfg = self.bert.cfg
        if bank.n_texts and bank.n_images:
            Lq = int(bank.img_feats.shape[1]) + int(bank.txt_ids.shape[1]) + 2
            if Lq > cfg.max_pos:
                raise ValueError(f"the bank's sequences hold {Lq} positions ([CLS] + regions + [SEP] + text), max_position_embeddings is "
                                 f"{cfg.max_pos}")
        cls_tok, input_txt, desc, segment, (feats, pos), sep_tok, lists = bank.assemble(idx, mode=mode, key=key, step=step, draws=draws)
        B = int(input_txt.shape[0])
        k = keep_count(B, drop_worst_ratio)
        if not 0 <= k <= B:
            raise ValueError(f"drop_worst_ratio {drop_worst_ratio} keeps {k} of {B} samples")
        dp = ops.report_plan(lists["masked_pos"], lists["masked_lm_labels"], lists["masked_weights"], desc.L, cfg.vocab_size,
                             valid_len=desc.desc[:, 2].contiguous() if self._pack(desc) else None)
        U, n, bad, _ = dp["counts"].tolist()
        if bad:
            raise ValueError(f"{bad} listed predictions are refused (report_finetune.build_plan: position 0, a position outside the "
                             "sequence or past the sample's valid length, a label outside the vocabulary, a negative or non-finite weight)")
        plan = dict(B=B, U=U, n=n, rows=dp["rows"][:U], row_ptr=dp["row_ptr"][:U + 1], labels=dp["labels"][:n], weights=dp["weights"][:n],
                    sample=dp["sample"][:n])
        return _ReportFn.apply(self, plan, k, cls_tok, input_txt, desc, segment, feats, pos, sep_tok, *self.bert._plist)

    def fit_step(self, bank, idx, optimizer, step, key=0, mode="s2s", drop_worst_ratio=0.0, draws=None):
        """One fine-tuning step (finetune.py:430-469) from a data.ReportBank: the masked batch of the items `idx` (one mv_report_assemble
        launch; (key, step) select the masking draw, `draws` overrides it), the row plan on the device, the objective, its backward
        (run_backward: an overflowed f16 backward is redone at a smaller loss scale) and optimizer.step().  `optimizer`: a
        medvill_amd.optim.BertAdam over model.parameters(); its gradients are cleared first.  mode: "s2s" / "bi" / "bar" or one per
        sample.  Returns the loss as a device scalar.  Refused: several ranks, an empty bank, a bank whose halves differ in size, a host
        idx outside the bank (IndexError), sequences longer than max_position_embeddings."""
        check_single_rank("CXRBertForReportFinetune", "data-parallel fine-tuning is not supported (drop-worst selects over the whole "
                          "batch and the gradients would not be all-reduced); fine-tune on one rank, or run eval_step")
        with self._engine_state("training", "keep_acts"):
            optimizer.zero_grad()
            with torch.enable_grad():
                self._prepare(True)
                loss = self._bank_loss(bank, idx, step, key, mode, drop_worst_ratio, draws)
                loss.backward()
        optimizer.step()
        return loss.detach()

    @torch.no_grad()
    def eval_step(self, bank, idx, step, key=0, mode="s2s", drop_worst_ratio=0.0, draws=None):
        """The loss of fit_step's batch in eval mode, without gradients; the engine's training / keep-activations / dropout-counter state
        is restored.  model.lm_stats holds the kept weight sum, sample count and argmax hits as after forward."""
        with self._engine_state("training", "keep_acts", "drop_counter") as eng:
            self._prepare(False)
            eng.training = False
            return self._bank_loss(bank, idx, step, key, mode, drop_worst_ratio, draws)

    def generate(self, cls_tok, input_img, sep_tok, **kw):
        """CXRBERT.generate of the weights being fine-tuned (validation decoding; eval mode, no gradients, engine state restored)."""
        return self.bert.generate(cls_tok, input_img, sep_tok, **kw)

    def evaluate(self, bank, idx=None, batch_size=64, **generate_kwargs):
        """Corpus BLEU-1..4 of the reports generated for the items of a data.ReportBank: report_eval.evaluate (DESIGN.md "8u")."""
        return report_eval.evaluate(self, bank, idx=idx, batch_size=batch_size, **generate_kwargs)

    # ------------------------------------------------------------------ state dict (the reference's fine-tune layout)
    def _apply(self, fn, *a, **k):
        self.bert._apply(fn, *a, **k)
        return self

    def state_dict(self, *a, **k):
        """finetune-style keys (checkpoint.to_finetune_keys: enc. -> '', mlm. -> cls.) of the CXRBERT state dict."""
        return to_finetune_keys(self.bert.state_dict())

    def load_state_dict(self, sd, strict=True):
        """A fine-tune-layout dict (state_dict above; finetune.py's checkpoints) or a CXRBERT pretraining dict (enc.* / mlm.* / itm.*)."""
        pretraining = any(k_.startswith("enc.") for k_ in sd)
        r = self.bert.load_state_dict(sd if pretraining else from_finetune_keys(sd), strict=False)
        if strict and (r.missing_keys or r.unexpected_keys):
            raise RuntimeError(f"load_state_dict: missing {r.missing_keys[:5]} unexpected {r.unexpected_keys[:5]}")
        return SimpleNamespace(missing_keys=list(r.missing_keys), unexpected_keys=list(r.unexpected_keys))

    def save_pretrained(self, save_directory):
        """config.json + pytorch_model.bin in the fine-tune layout; CXRBERT.from_pretrained / CXRBertForGeneration.from_pretrained
        read it back."""
        write_pretrained(save_directory, hf_config(self.bert.cfg, "CXRBertForReportFinetune", label_smoothing=self.label_smoothing),
                         self.state_dict())

    @classmethod
    def from_pretrained(cls, path_or_state_dict, config=None, args=None, label_smoothing=None, **kw):
        """A checkpoint directory (CXRBERT.save_pretrained or save_pretrained above) or a state dict (then `config` is required)."""
        config, sd = read_pretrained(path_or_state_dict, config)
        m = cls(config, args, label_smoothing=label_smoothing, **kw)
        m.load_state_dict(sd, strict=False)
        return m
