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

import json
import os
import weakref
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import hip_ops as ops
from ._lib import EPI_BIAS, EPI_BIAS_RELU, MV_F16, MV_F32
from .checkpoint import from_finetune_keys, to_finetune_keys
from .cxrbert import CXRBERT, _hand_over_grads, _holds_views, _use_views

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


def _check_single_rank():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError("CXRBertForVQA: data-parallel VQA fine-tuning is not supported (the classifier's gradients would not be "
                           "all-reduced); fine-tune on one rank, or run inference under torch.no_grad()")


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
        bert = model.bert
        eng = bert.engine
        # gradients an earlier backward left in the flat buffers THROUGH the .grad views: kept and added to, like autograd would
        views = _use_views(bert)
        held = eng.flat_g.clone() if (views and eng.flat_g is not None and _holds_views(bert)) else None
        held_h = model.head_g.clone() if (views and model.head_g is not None and model._head_holds_views()) else None
        model._backward_once(ctx, g)
        if eng.scaler is not None:
            # f16 gradient operands under a loss scale (as _CXRBertFn.backward): an overflow -- the classifier's gradients included -- is
            # redone with a smaller scale, because the gradients go to an optimizer that cannot skip the step
            for _ in range(8):
                eng.scaler[6:7].zero_()
                ops.count_nonfinite(eng.flat_g, eng.scaler[6:7])
                ops.count_nonfinite(model.head_g, eng.scaler[6:7])
                if float(eng.scaler[6]) == 0.0:
                    break
                eng.reset_scaler(max(float(eng.scaler[0]) / 16.0, 1.0))
                model._backward_once(ctx, g)
        if held is not None:
            eng.flat_g.add_(held)
        if held_h is not None:
            model.head_g.add_(held_h)
        return (None,) * 11 + _hand_over_grads(bert) + model._hand_over_head(views)


class CXRBertForVQA(nn.Module):
    """`BertForPreTrainingLossMask(config, args, tasks='vqa')` with this package's CXRBERT input convention:
        forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, ans_labels=None, ans_type=None, vqa_inference=False)
          ans_labels (soft targets f32 [B, A], data_loader.py:255-272) -> (dummy zero [1], mean BCE loss); model.vqa_stats =
              f32[6] device [score_sum, bce_sum, closed_score, closed_n, open_score, open_n] (ans_type 0 = CLOSED, 1 = OPEN),
              model.vqa_pred = argmax over all answers (int64 [B])
          vqa_inference=True -> ans_idx int64 [B] = argmax(classifier([CLS] (.) [SEP])[:, 1:]) + 1   (model.py:979-983)
          neither -> differentiable logits [B, A] of the [CLS] row
    .bert is the CXRBERT; .ans_classifier the Sequential(Linear, ReLU, Linear) whose Parameters are views of the classifier's flat buffer.
    `attn_mask` may be a materialised mask or data.MaskDesc descriptors (16-bit: the encoder then runs on the valid rows only)."""

    # medvill_amd.optim.BertAdam: the classifier's tensors, and the encoder tensors the VQA graph never reaches (`grad is None` in the
    # reference: no update, no weight decay)
    _head_keys = HEAD_KEYS
    _padded_key = HEAD_KEYS[2]            # the weight whose rows are padded to Ap inside the flat buffer
    _unreached = ("mlm.", "itm.", "enc.pooler.")

    def __init__(self, config, args=None, n_answers=N_ANSWERS, **kw):
        super().__init__()
        self.bert = CXRBERT(config, args, **kw)
        self._init_head(int(n_answers))

    def _init_head(self, A):
        eng = self.bert.engine
        H = self.bert.cfg.hidden
        self.n_answers = A
        self._layout, self._n_head, self.Ap = head_layout(H, A)
        dev = eng.device
        self.head_p = torch.zeros(self._n_head, dtype=torch.float32, device=dev)
        self.head_g = self.head_m = self.head_v = None
        # 16-bit copies in the encodings the engine uses (the same rule as Engine.shadow / shadow_f)
        self.head_sh = torch.zeros(self._n_head, dtype=torch.bfloat16, device=dev) if eng.shadow is not None else None
        self.head_shf = torch.zeros(self._n_head, dtype=torch.float16, device=dev) if eng.shadow_f is not None else None
        self.ans_classifier = nn.Sequential(nn.Linear(H, 2 * H), nn.ReLU(), nn.Linear(2 * H, A))
        self._hplist = []
        for name in self._head_keys:
            idx, leaf = name.split(".")[1:]
            par = nn.Parameter(self._view(self.head_p, name), requires_grad=True)
            par._medvill_head = weakref.ref(self)          # medvill_amd.optim.AdamW finds the classifier's flat buffers through it
            self.ans_classifier[int(idx)]._parameters[leaf] = par
            self._hplist.append(par)
        self._head_versions = None
        self._acts = None
        self.vqa_stats = self.vqa_pred = None
        self.reset_head()

    # ------------------------------------------------------------------ classifier storage
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
        # .to(device) / .cuda(): the encoder moves its flat buffers (CXRBERT._apply), the classifier its own; the Parameters stay views
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

    def _sync_head(self):
        """16-bit copies of the classifier from its fp32 master (after an outside optimizer or a load changed the Parameters)."""
        for sh in (self.head_sh, self.head_shf):
            if sh is not None:
                ops.cast(self.head_p, sh, self._n_head)
        self._head_versions = sum(p._version for p in self._hplist)

    def _head_holds_views(self):
        return any(p.grad is not None and p.grad.data_ptr() == self._view(self.head_g, n).data_ptr() for n, p in zip(self._head_keys, self._hplist))

    def _hand_over_head(self, views):
        """The classifier's gradients -> torch, by the rule of cxrbert._hand_over_grads (views of the flat gradient unless a hook or a
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
    def _prepare(self, want_grad):
        bert = self.bert
        eng = bert.engine
        # Parameters stepped by an outside optimizer (or loaded): refresh the 16-bit copies -- unless medvill_amd.optim.AdamW, whose
        # kernels write them, was the last to touch them (version counters, as CXRBERT's forward)
        if not bert.__dict__.pop("_shadow_fresh", False):
            eng.shadow_dirty = eng.shadow_dirty or bert._params_dirty()
        if eng.is16 and self._head_dirty():
            self._sync_head()
        eng.training = self.training             # encoder dropout only in train mode; the classifier has none
        eng.keep_acts = bool(want_grad)          # under torch.no_grad() nothing is saved for a backward

    def _encode_and_classify(self, cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, infer):
        """Encoder (last layer on the consumed rows) + classifier -> logits [B, Ap] f32 (columns A..Ap-1 unspecified).
        Training vector: the [CLS] row (model.py:1021); inference: [CLS] (.) the image [SEP] row N+1 (model.py:980)."""
        from .data import MaskDesc
        eng = self.bert.engine
        dev = eng.device
        B, N = int(input_txt.shape[0]), int(feats.shape[1])
        Lq = N + int(input_txt.shape[1]) + 2
        pack = isinstance(attn_mask, MaskDesc) and eng.is16 and attn_mask.packable()
        ar = torch.arange(B, device=dev, dtype=torch.int32)
        # tail_rows: none for training (the compact final state is the B [CLS] rows); the image [SEP] rows for inference (then
        # [SEP rows | CLS rows])
        tail = ar * Lq + (N + 1) if infer else ar[:0]
        eng.encoder_forward(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, pack=pack, tail_rows=tail)
        S, H = eng.S, self.bert.cfg.hidden
        if infer:
            x = eng._buf("vqa_emb", (B, H), eng.fadt)
            ops.rows_mul(S["hidden_f"], ar + B, S["hidden_f"], ar, x, R=B, H=H)
            xb = None
        else:
            x, xb = S["hidden_f"][:B], S["hidden"][:B]
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
        if self.head_g is None:
            self.head_g = torch.zeros_like(self.head_p)
        else:
            self.head_g.zero_()
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
        dx = eng._buf("dhidden_tail", (B, H), adt)
        ops.gemm(dz, self._view(w, HEAD_KEYS[0]), dx, tb=True, M=B, N=H, K=2 * H, lda=2 * H, ldb=H)
        eng.S["dhidden"] = dx                     # the compact final state's gradient: the pooler / ITM / MLM heads get none
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
            _check_single_rank()
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
        self._prepare(want_grad)
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
        eng = self.bert.engine
        prev = (eng.training, eng.keep_acts)
        try:
            self._prepare(False)
            logits = self._encode_and_classify(cls_tok, input_txt, attn_mask, segment, feats, pos, sep_tok, infer=True)
            ans = torch.empty(int(input_txt.shape[0]), dtype=torch.int64, device=eng.device)
            ops.bce_fwd_bwd(logits, self.n_answers, ld=self.Ap, arg_infer=ans)
        finally:                # sticky engine state: a later direct Engine user must find what it left
            eng.training, eng.keep_acts = prev
        return ans

    # ------------------------------------------------------------------ optimizer hook (medvill_amd.optim.AdamW)
    def _adamw_head(self, step, lr, betas, eps, weight_decay, correct_bias):
        grads = [p.grad for p in self._hplist]
        if all(g is None for g in grads):
            return
        if any(g is None for g in grads):
            raise RuntimeError("some classifier Parameters have a gradient and some have none: the flat update cannot skip individual tensors")
        if self.head_g is None:
            self.head_g = torch.zeros_like(self.head_p)
        for name, g in zip(self._head_keys, grads):
            gv = self._view(self.head_g, name)
            if g.data_ptr() != gv.data_ptr():
                gv.copy_(g)
        if self.head_m is None:
            self.head_m, self.head_v = torch.zeros_like(self.head_p), torch.zeros_like(self.head_p)
        ops.adamw_step(self.head_p, self.head_g, self.head_m, self.head_v, self.head_sh, self._n_head, lr, betas[0], betas[1], eps,
                       weight_decay, step, correct_bias, 1.0, shadow_f16=self.head_shf)
        self._head_versions = sum(p._version for p in self._hplist)      # the kernel has written the 16-bit copies too

    # ------------------------------------------------------------------ state dict (the reference's VQA layout)
    def state_dict(self, *a, **k):
        """finetune-style keys (checkpoint.to_finetune_keys) of the encoder -- no cls.* / itm.* (the VQA model has no MLM / ITM head)
        -- plus ans_classifier.{0,2}.{weight,bias}."""
        sd = self.bert.state_dict()
        out = to_finetune_keys(OrderedDict((k_, v) for k_, v in sd.items() if not k_.startswith(("mlm.", "itm."))))
        for name, p in zip(HEAD_KEYS, self._hplist):
            out[name] = p.detach().clone()
        return out

    def load_state_dict(self, sd, strict=True):
        """A VQA-layout dict (finetune keys + ans_classifier.*) or a CXRBERT pretraining state dict (enc.* / mlm.* / itm.*; the
        classifier then starts from reset_head())."""
        head = {k_: v for k_, v in sd.items() if k_.startswith("ans_classifier.")}
        rest = OrderedDict((k_, v) for k_, v in sd.items() if not k_.startswith("ans_classifier."))
        pretraining = any(k_.startswith("enc.") for k_ in rest)
        r = self.bert.load_state_dict(rest if pretraining else from_finetune_keys(rest), strict=False)
        missing = [k_ for k_ in r.missing_keys if not k_.startswith(("mlm.", "itm."))]
        unexpected = list(r.unexpected_keys) + [k_ for k_ in head if k_ not in HEAD_KEYS]
        with torch.no_grad():
            if head:
                for name in HEAD_KEYS:
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

    def save_pretrained(self, save_directory):
        """config.json + pytorch_model.bin in the reference's VQA layout."""
        os.makedirs(save_directory, exist_ok=True)
        c = self.bert.cfg
        cj = dict(architectures=["CXRBertForVQA"], model_type="bert", vocab_size=c.vocab_size, hidden_size=c.hidden,
                  num_hidden_layers=c.layers, num_attention_heads=c.heads, intermediate_size=c.intermediate,
                  max_position_embeddings=c.max_pos, type_vocab_size=c.type_vocab, layer_norm_eps=c.ln_eps, hidden_act="gelu",
                  hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, n_answers=self.n_answers)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(cj, f, indent=2)
        torch.save({k_: v.cpu() for k_, v in self.state_dict().items()}, os.path.join(save_directory, "pytorch_model.bin"))

    @classmethod
    def from_pretrained(cls, path_or_state_dict, config=None, args=None, n_answers=None, **kw):
        """A checkpoint directory (config.json + pytorch_model.bin: CXRBERT.save_pretrained or save_pretrained above) or a state dict
        (then `config` is required) -> model.  A pretraining checkpoint initialises the classifier from torch.initial_seed()."""
        if isinstance(path_or_state_dict, (str, os.PathLike)):
            if config is None:
                with open(os.path.join(path_or_state_dict, "config.json")) as f:
                    config = json.load(f)
            sd = torch.load(os.path.join(path_or_state_dict, "pytorch_model.bin"), map_location="cpu")
        else:
            sd = path_or_state_dict
            if config is None:
                raise ValueError("from_pretrained(state_dict): pass config= as well")
        if n_answers is None:
            w = sd.get(HEAD_KEYS[2])
            n_answers = int(w.shape[0]) if w is not None else int(config.get("n_answers", N_ANSWERS) if isinstance(config, dict) else N_ANSWERS)
        m = cls(config, args, n_answers=n_answers, **kw)
        m.load_state_dict(sd, strict=False)
        return m
