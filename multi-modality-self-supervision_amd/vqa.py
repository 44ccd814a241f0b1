"""Medical VQA fine-tuning and answer prediction on the HIP engine: the reference's `BertForPreTrainingLossMask(tasks='vqa')`
(Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:903-1054) on top of a pretrained CXRBERT.

    model = CXRBertForVQA.from_pretrained(ckpt_dir)                          # finetune.py:338-339 (enc. -> '', mlm. -> cls.)
    _, loss = model(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, ans_labels=target, ans_type=ans_type)
    loss.backward(); optimizer.step()                                        # finetune.py:443-451
    ans_idx = model(..., vqa_inference=True)                                 # model.py:979-983

The answer classifier is Linear(H, 2H) + ReLU + Linear(2H, A) (model.py:939-943) over the last layer's [CLS] row in training and over
[CLS] (.) image-[SEP] at inference, as in the reference (the two paths feed it different vectors: mirrored, not unified).  The encoder runs
its last layer's per-row work on the rows the classifier reads only (Engine.encoder_forward, tail_rows); the classifier's products,
BCEWithLogits, its gradient and the score split are HIP kernels (mv_gemm_rows / mv_gemm, mv_bce_fwd_bwd, mv_dact mode 2, mv_rows_mul).
The classifier's parameters live in a small flat buffer of their own (fp32 master + the 16-bit copies the kernels read), which
medvill_amd.optim.AdamW / BertAdam update with one more fused launch.  Arithmetic is CXRBERT's (the pretrained model), DESIGN.md "8b. VQA".
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from . import hip_ops as ops
from ._lib import EPI_BIAS, EPI_BIAS_RELU
from .checkpoint import from_finetune_keys, hf_config, read_pretrained, to_finetune_keys, write_pretrained
from .cxrbert import run_backward
from .task import FlatHead, check_single_rank

N_ANSWERS = 458          # model.py:942
HEAD_KEYS = ("ans_classifier.0.weight", "ans_classifier.0.bias", "ans_classifier.2.weight", "ans_classifier.2.bias")
_ROWS = 256              # mv_gemm_rows takes at most 256 rows per launch


def head_layout(H: int, A: int):
    """name -> (offset, shape) of the classifier's flat buffer, its size and the padded answer count Ap (A rounded up to 16).  The
    second layer's weight / bias own Ap rows: rows A..Ap-1 stay zero (no gradient ever reaches them), so the 16-bit copy of the whole
    buffer holds the [Ap, 2H] operand the padded products read and the optimizer's kernel writes it in place."""
    Ap = (A + 15) // 16 * 16
    lay, off = OrderedDict(), 0
    for name, shape, n in ((HEAD_KEYS[0], (2 * H, H), 2 * H * H), (HEAD_KEYS[1], (2 * H,), 2 * H), (HEAD_KEYS[2], (A, 2 * H), Ap * 2 * H),
                           (HEAD_KEYS[3], (A,), Ap)):
        lay[name] = (off, shape)
        off += (n + 63) // 64 * 64
    return lay, off, Ap


def vqa_metrics(counters) -> dict:
    """mv_vqa_score's integer counters [G, 3, 2] = {sum of fx(score), samples} by group and type slot (closed, open, neither) -> the
    reference's numbers, formed in f64 from exact integer sums: dict(acc, closed_acc, open_acc, n, closed_n, open_n, by_group {g: the
    same six, for the groups that have samples}).  acc counts every sample, the two splits their own; a split without samples is nan."""
    c = torch.as_tensor(counters).to(torch.int64).reshape(-1, 3, 2).tolist()

    def ratio(fx, cnt):
        return fx / 4294967296.0 / cnt if cnt else float("nan")

    def six(groups):
        fx = [sum(g[t][0] for g in groups) for t in range(3)]
        cnt = [sum(g[t][1] for g in groups) for t in range(3)]
        return dict(acc=ratio(sum(fx), sum(cnt)), closed_acc=ratio(fx[0], cnt[0]), open_acc=ratio(fx[1], cnt[1]), n=sum(cnt),
                    closed_n=cnt[0], open_n=cnt[1])

    out = six(c)
    out["by_group"] = {g: six([row]) for g, row in enumerate(c) if sum(t[1] for t in row)}
    return out


class _VQAFn(torch.autograd.Function):
    """Encoder + answer classifier (+ BCE) as one autograd node.  mode "loss": -> mean BCE (the reference's vqa_loss); mode "logits":
    -> logits [B, A].  The backward runs the classifier's backward into the compact [B, H] hidden-state gradient, then the encoder's."""

    @staticmethod
    def forward(ctx, model, mode, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, target, ans_type, *params):
        eng = model.bert.engine
        B, A = int(input_txt.shape[0]), model.n_answers
        logits = model._encode_and_classify(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, infer=False)
        ctx.model, ctx.mode, ctx.B = model, mode, B
        ctx.acts = model._acts
        if mode == "logits":
            return logits[:, :A].clone()
        stats = torch.zeros(6, dtype=torch.float32, device=eng.device)
        pred = torch.empty(B, dtype=torch.int64, device=eng.device)
        ops.bce_fwd_bwd(logits, A, R=B, ld=model.Ap, target=target, ans_type=ans_type, stats=stats, arg_train=pred)
        model.vqa_stats, model.vqa_pred = stats, pred
        ctx.target = target
        return stats[1] / float(B * A)          # BCEWithLogitsLoss(): the mean over B * A elements

    @staticmethod
    def backward(ctx, g):
        model = ctx.model
        return (None,) * 11 + run_backward(model.bert, lambda: model._backward_once(ctx, g), head=model)


class CXRBertForVQA(FlatHead):
    """`BertForPreTrainingLossMask(config, args, tasks='vqa')` with this package's CXRBERT input convention:
        forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, ans_labels=None, ans_type=None, vqa_inference=False)
          ans_labels (soft targets f32 [B, A], data_loader.py:255-272) -> (dummy zero [1], mean BCE loss); model.vqa_stats =
              f32[6] device [score_sum, bce_sum, closed_score, closed_n, open_score, open_n] (ans_type 0 = CLOSED, 1 = OPEN),
              model.vqa_pred = argmax over all answers (int64 [B])
          vqa_inference=True -> ans_idx int64 [B] = argmax(classifier([CLS] (.) [SEP])[:, 1:]) + 1   (model.py:979-983)
          neither -> differentiable logits [B, A] of the [CLS] row
    .bert is the CXRBERT; .ans_classifier the Sequential(Linear, ReLU, Linear) whose Parameters are views of the classifier's flat buffer
    (task.FlatHead).
    `attn_mask` may be a materialised mask or data.MaskDesc descriptors (16-bit: the encoder then runs on the valid rows only).
    fit_step / evaluate: the same step, and the reference's whole-set evaluation with its closed / open split, from a device-resident
    data.VqaBank -- the batch built by one HIP launch, one read-back per evaluation (DESIGN.md "8r")."""

    # medvill_amd.optim.BertAdam: the classifier's tensors, and the encoder tensors the VQA graph never reaches (`grad is None` in the
    # reference: no update, no weight decay)
    _head_keys = HEAD_KEYS
    _padded_key = HEAD_KEYS[2]            # the weight whose rows are padded to Ap inside the flat buffer
    _unreached = ("mlm.", "itm.", "enc.pooler.")

    def __init__(self, config, args=None, n_answers=N_ANSWERS, **kw):
        super().__init__(config, args, **kw)
        H, A = self.bert.cfg.hidden, int(n_answers)
        self.n_answers = A
        self.ans_classifier = nn.Sequential(nn.Linear(H, 2 * H), nn.ReLU(), nn.Linear(2 * H, A))
        self._acts = None
        self.vqa_stats = self.vqa_pred = None
        self._init_head(head_layout(H, A))

    @torch.no_grad()
    def reset_head(self, seed: int | None = None):
        """init_bert_weights (model.py:930): weights N(0, 0.02), biases zero; seeded from torch.initial_seed() unless `seed` is given."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(torch.initial_seed() if seed is None else seed)
        flat = torch.zeros(self._n_head, dtype=torch.float32)
        for name in HEAD_KEYS:
            if name.endswith("weight"):
                v = self._view(flat, name)
                v.copy_(torch.randn(v.shape, generator=gen) * 0.02)
        self.head_p.copy_(flat.to(self.head_p.device))
        self._head_versions = None

    # ------------------------------------------------------------------ forward
    def _encode_and_classify(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, infer):
        """Encoder (last layer on the consumed rows) + classifier -> logits [B, Ap] f32 (columns A..Ap-1 unspecified).
        Training vector: the [CLS] row (model.py:1021); inference: [CLS] (.) the image [SEP] row N+1 (model.py:980)."""
        eng = self.bert.engine
        B, N = int(input_txt.shape[0]), int(feats.shape[1])
        H = self.bert.cfg.hidden
        # tail_rows: none for training (the compact final state is the B [CLS] rows); the image [SEP] rows for inference (then
        # [SEP rows | CLS rows])
        if infer:
            ar = torch.arange(B, device=eng.device, dtype=torch.int32)
            eng.encoder_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, pack=self._pack(attn_mask),
                                tail_rows=ar * (N + int(input_txt.shape[1]) + 2) + (N + 1))
            S = eng.S
            x = eng._buf("vqa_emb", (B, H), eng.fadt)
            ops.rows_mul(S["hidden_f"], ar + B, S["hidden_f"], ar, x, R=B, H=H)
            xb = None
        else:
            self.encode_cls_rows(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok)
            x, xb = eng.S["hidden_f"][:B], eng.S["hidden"][:B]
        return self._classify(x, xb, B)

    def _classify(self, x, xb, B):
        eng = self.bert.engine
        H, A, Ap = self.bert.cfg.hidden, self.n_answers, self.Ap
        wf = self._shadow_of(eng.fdt)
        b1, b2 = self._view(self.head_p, HEAD_KEYS[1]), self._view(self.head_p, HEAD_KEYS[3])
        W1, W2 = self._view(wf, HEAD_KEYS[0]), self._view(wf, HEAD_KEYS[2], padded=True)
        h1 = eng._buf("vqa_h1", (B, 2 * H), eng.fadt)
        logits = eng._buf("vqa_logits", (B, Ap), torch.float32)
        if eng.is16:
            for r0 in range(0, B, _ROWS):
                m = min(_ROWS, B - r0)
                ops.gemm_rows(x[r0:r0 + m], W1, h1[r0:r0 + m], M=m, N=2 * H, K=H, bias=b1, epi=EPI_BIAS_RELU)
            for r0 in range(0, B, _ROWS):
                m = min(_ROWS, B - r0)
                ops.gemm_rows(h1[r0:r0 + m], W2, logits[r0:r0 + m], M=m, N=A, K=2 * H, ldc=Ap, bias=b2, epi=EPI_BIAS)
        else:
            ops.gemm(x, W1, h1, M=B, N=2 * H, K=H, bias=b1, epi=EPI_BIAS_RELU)
            ops.gemm(h1, W2, logits, M=B, N=A, K=2 * H, ldc=Ap, bias=b2, epi=EPI_BIAS)
        if xb is not None:
            h1b = h1
            if eng.dual:                          # the gradient products read the other 16-bit encoding
                h1b = eng._buf("vqa_h1_b", (B, 2 * H), eng.adt)
                ops.cast(h1, h1b, B * 2 * H)
            self._acts = dict(x=xb, h1=h1b, logits=logits)
        return logits

    def _backward_once(self, ctx, g):
        bert = self.bert
        eng = bert.engine
        B, A, Ap, H = ctx.B, self.n_answers, self.Ap, bert.cfg.hidden
        acts = ctx.acts
        eng.zero_grad()
        self._zero_head_grad()
        adt, us = eng.adt, eng.unscale_dev
        dl = eng._buf("vqa_dlogits", (B, Ap), adt)
        if ctx.mode == "loss":
            gs = g.detach().to(eng.device, torch.float32).reshape(1) / float(B * A)      # d(mean) = upstream / (B * A), on the device
            ops.bce_fwd_bwd(acts["logits"], A, R=B, ld=Ap, target=ctx.target, dgrad=dl, ldd=Ap, grad_scale_dev=gs,
                            loss_scale_dev=eng.loss_scale_dev)
        else:
            d32 = g.detach().to(eng.device, torch.float32).contiguous()
            ls = eng.loss_scale_dev               # f16 gradients: the incoming f32 gradient enters the chain multiplied by S
            ops.cast2d(d32 if ls is None else d32 * ls, A, dl, Ap, B, A)
        w = self._shadow_of(eng.dt)
        gW1, gb1 = self._view(self.head_g, HEAD_KEYS[0]), self._view(self.head_g, HEAD_KEYS[1])
        gW2, gb2 = self._view(self.head_g, HEAD_KEYS[2]), self._view(self.head_g, HEAD_KEYS[3])
        # second layer: db2, dW2 = dl^T . h1, dh1 = dl . W2 (contraction over the padded Ap columns: the padding of dl is zero)
        ops.colsum(dl, Ap, B, A, gb2, accumulate=True, unscale=us)
        eng._dW(dl, acts["h1"], gW2, A, 2 * H, B, lda=Ap, ldb=2 * H)
        dh1 = eng._buf("vqa_dh1", (B, 2 * H), adt)
        ops.gemm(dl, self._view(w, HEAD_KEYS[2], padded=True), dh1, tb=True, M=B, N=2 * H, K=Ap, lda=Ap, ldb=2 * H)
        # ReLU backward on the saved output, then the first layer
        dz = eng._buf("vqa_dz", (B, 2 * H), adt)
        ops.dact(2, dh1, acts["h1"], dz, B * 2 * H)
        ops.colsum(dz, 2 * H, B, 2 * H, gb1, accumulate=True, unscale=us)
        eng._dW(dz, acts["x"], gW1, 2 * H, H, B, lda=2 * H, ldb=H)
        dx = eng.dhidden_buffer()                 # the compact final state's gradient: the pooler / ITM / MLM heads get none
        ops.gemm(dz, self._view(w, HEAD_KEYS[0]), dx, tb=True, M=B, N=H, K=2 * H, lda=2 * H, ldb=H)
        eng.encoder_backward()

    def forward(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, ans_labels=None, ans_type=None, vqa_inference=False):
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError            # model.py:956-961
        feats, pos = self.bert._regions(input_img)
        if vqa_inference:
            if ans_labels is not None:
                raise ValueError("vqa_inference=True takes no ans_labels (model.py:979)")
            return self.predict(cls_tok, input_txt, attn_mask, segment, (feats, pos), sep_tok)
        want_grad = torch.is_grad_enabled()
        if want_grad:
            check_single_rank("CXRBertForVQA", "data-parallel VQA fine-tuning is not supported (the classifier's gradients would not be "
                              "all-reduced); fine-tune on one rank, or run inference under torch.no_grad()")
        eng = self.bert.engine
        B, A = int(input_txt.shape[0]), self.n_answers
        target = at = None
        if ans_labels is not None:
            target = torch.as_tensor(ans_labels).to(eng.device, torch.float32).contiguous()
            if tuple(target.shape) != (B, A):
                raise ValueError(f"ans_labels must be the soft target [B, A] = [{B}, {A}], got {tuple(target.shape)}")
            if ans_type is not None:
                at = torch.as_tensor(ans_type).to(eng.device, torch.int32).reshape(-1).contiguous()
                if at.numel() != B:
                    raise ValueError("ans_type must hold one entry per sample")
        self._prepare(want_grad)                 # (engine state NOT restored after the call; CXRBertForReportFinetune.forward restores it)
        params = list(self.bert._plist) + self._hplist
        if target is None:
            return _VQAFn.apply(self, "logits", cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, None, None, *params)
        loss = _VQAFn.apply(self, "loss", cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, target, at, *params)
        return loss.new_zeros(1), loss           # (dummy_value, vqa_loss), model.py:1014,1041

    @torch.no_grad()
    def predict(self, cls_tok, input_txt, attn_mask, segment, input_img, sep_tok):
        """ans_idx int64 [B] = argmax(ans_classifier(seq[:, 0] * seq[:, N + 1])[:, 1:]) + 1 (model.py:979-983)."""
        if attn_mask.dim() not in (2, 3):
            raise NotImplementedError
        feats, pos = self.bert._regions(input_img)
        with self._engine_state("training", "keep_acts") as eng:
            self._prepare(False)
            logits = self._encode_and_classify(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, infer=True)
            ans = torch.empty(int(input_txt.shape[0]), dtype=torch.int64, device=eng.device)
            ops.bce_fwd_bwd(logits, self.n_answers, ld=self.Ap, arg_infer=ans)
        return ans

    # ------------------------------------------------------------------ steps from a device-resident bank
    def _check_bank(self, bank):
        if bank.n_questions == 0 or bank.n_images == 0:
            raise ValueError("the bank is empty (VqaBank.add_questions, add_images)")
        if bank.n_answers != self.n_answers:
            raise ValueError(f"the bank holds targets over {bank.n_answers} answers, the classifier has {self.n_answers}")
        Lq = int(bank.img_feats.shape[1]) + int(bank.txt_ids.shape[1]) + 2
        if Lq > self.bert.cfg.max_pos:
            raise ValueError(f"the bank's sequences hold {Lq} positions ([CLS] + regions + [SEP] + text), max_position_embeddings is "
                             f"{self.bert.cfg.max_pos}")

    def fit_step(self, bank, idx, optimizer, mode="bi"):
        """One fine-tuning step (finetune.py:430-469, tasks='vqa') from a data.VqaBank: optimizer.zero_grad(), the batch of the questions
        `idx` (one mv_vqa_assemble launch), the loss node of forward, its backward and optimizer.step().  mode: "s2s" / "bi" / "bar" or
        one per sample.  Returns the loss as a device scalar; vqa_stats / vqa_pred are set as after forward.  Refused: several ranks,
        an empty bank, a bank over another answer count, sequences longer than max_position_embeddings, a host idx outside the bank
        (IndexError)."""
        check_single_rank("CXRBertForVQA", "data-parallel VQA fine-tuning is not supported (the classifier's gradients would not be "
                          "all-reduced); fine-tune on one rank, or run evaluate")
        self._check_bank(bank)
        with self._engine_state("training", "keep_acts"):
            optimizer.zero_grad()
            with torch.enable_grad():
                cls_tok, input_txt, desc, segment, img, sep_tok, target, ans_type = bank.assemble(idx, mode=mode)
                _, loss = self(cls_tok, input_txt, desc, segment, img, sep_tok, ans_labels=target, ans_type=ans_type)
                loss.backward()
        optimizer.step()
        return loss.detach()

    @torch.no_grad()
    def evaluate(self, bank, idx=None, batch_size=64, path="inference", mode="bi"):
        """The reference's evaluation over the questions `idx` of a data.VqaBank (None: every question, in order), in eval mode and
        without gradients; a last partial batch is allowed.  path "inference": the [CLS] (.) image-[SEP] vector and the argmax over
        columns 1.. (model.py:979-983); "train": the [CLS] vector, the argmax over all columns and the BCE sum (model.py:1020-1023).
        Every batch's predictions go into one device buffer, one mv_vqa_score launch scores them against the bank's sparse answers and
        sums them by group and closed / open split; ONE read-back at the end.  -> dict(acc, closed_acc, open_acc, n, closed_n, open_n,
        by_group {g: the same six numbers, for the groups that have samples}, loss (path "train": the mean BCE over n * A elements),
        pred int64 [n] and score f32 [n] on the device).  A split without samples has accuracy nan.  The engine's training /
        keep-activations / dropout-counter state is restored."""
        if path not in ("inference", "train"):
            raise ValueError(f"path {path!r}: 'inference' or 'train'")
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
            take = bank.host_idx(torch.arange(bank.n_questions) if idx is None else idx)
            dev_idx = take.to(torch.int32).to(eng.device)
        n, A, bs = int(dev_idx.numel()), self.n_answers, int(batch_size)
        if not isinstance(mode, str) and len(mode) != n:
            raise ValueError(f"mode: one name, or one per question ({n})")
        pred = torch.empty(n, dtype=torch.int64, device=eng.device)
        stats = torch.zeros(6, dtype=torch.float32, device=eng.device)
        with self._engine_state("training", "keep_acts", "drop_counter"):
            self._prepare(False)
            eng.training = False
            for s in range(0, n, bs):
                e = min(n, s + bs)
                cls_tok, input_txt, desc, segment, (feats, pos), sep_tok, target, ans_type = bank.assemble(
                    take[s:e], mode=mode if isinstance(mode, str) else list(mode[s:e]))
                logits = self._encode_and_classify(cls_tok, input_txt, desc, segment, feats, pos, sep_tok, infer=path == "inference")
                if path == "inference":
                    ops.bce_fwd_bwd(logits, A, R=e - s, ld=self.Ap, arg_infer=pred[s:e])
                else:
                    ops.bce_fwd_bwd(logits, A, R=e - s, ld=self.Ap, target=target, ans_type=ans_type, stats=stats, arg_train=pred[s:e])
            score, counters = ops.vqa_score(pred, dev_idx, bank.ans_ptr, bank.ans_label, bank.ans_score, bank.ans_type, group=bank.group)
        # the one read-back: the integer counters and the bits of the f32 BCE sum
        host = torch.cat([counters.reshape(-1), stats.view(torch.int32).to(torch.int64)]).cpu()
        out = vqa_metrics(host[:counters.numel()].view(-1, 3, 2))
        if path == "train":
            k = counters.numel() + 1                      # stats[1]: the BCE sum
            out["loss"] = float(host[k:k + 1].to(torch.int32).view(torch.float32)) / float(n * A)
        out["pred"], out["score"] = pred, score
        return out

    # ------------------------------------------------------------------ state dict (the reference's VQA layout)
    def state_dict(self, *a, **k):
        """finetune-style keys (checkpoint.to_finetune_keys) of the encoder -- no cls.* / itm.* (the VQA model has no MLM / ITM head)
        -- plus ans_classifier.{0,2}.{weight,bias}."""
        sd = self.bert.state_dict()
        out = to_finetune_keys(OrderedDict((k_, v) for k_, v in sd.items() if not k_.startswith(("mlm.", "itm."))))
        return self._head_state(out)

    def load_state_dict(self, sd, strict=True):
        """A VQA-layout dict (finetune keys + ans_classifier.*) or a CXRBERT pretraining state dict (enc.* / mlm.* / itm.*; the
        classifier then starts from reset_head())."""
        head = {k_: v for k_, v in sd.items() if k_.startswith("ans_classifier.")}
        rest = OrderedDict((k_, v) for k_, v in sd.items() if not k_.startswith("ans_classifier."))
        pretraining = any(k_.startswith("enc.") for k_ in rest)
        return self._load_state(head, rest if pretraining else from_finetune_keys(rest), strict)

    def save_pretrained(self, save_directory):
        """config.json + pytorch_model.bin in the reference's VQA layout."""
        write_pretrained(save_directory, hf_config(self.bert.cfg, "CXRBertForVQA", n_answers=self.n_answers), self.state_dict())

    @classmethod
    def from_pretrained(cls, path_or_state_dict, config=None, args=None, n_answers=None, **kw):
        """A checkpoint directory (config.json + pytorch_model.bin: CXRBERT.save_pretrained or save_pretrained above) or a state dict
        (then `config` is required) -> model.  A pretraining checkpoint initialises the classifier from torch.initial_seed()."""
        config, sd = read_pretrained(path_or_state_dict, config)
        if n_answers is None:
            w = sd.get(HEAD_KEYS[2])
            n_answers = int(w.shape[0]) if w is not None else int(config.get("n_answers", N_ANSWERS) if isinstance(config, dict) else N_ANSWERS)
        m = cls(config, args, n_answers=n_answers, **kw)
        m.load_state_dict(sd, strict=False)
        return m
