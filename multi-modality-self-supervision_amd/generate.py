"""KV-cached report generation on the HIP engine (DESIGN.md "Generation").

Generation is iterated CXRBERT.forward under the seq2seq mask in eval mode (`s2s`): the prefix
[CLS] + N regions + [SEP] (segment 0) only sees itself, so its keys / values are computed once (prefill: the engine's own
full-attention forward over n2 = N + 2 rows); text token t sits at position t with segment 1.  Decode step t feeds two rows per
beam -- y_{t-1} at position t-1 (not at t = 0) and [MASK] at position t -- each attending to the prefix, the cached text rows
before it and itself; y_t is read from the MLM head at the MASK row (UniLM's scheme, the reference's
Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:1132-1487).

Cache: per layer one [slots, 2H] matrix (K | V) in the forward operand encoding.  Slots: the prefix of sample b at b*n2 + i;
text token at position p of beam r at B*n2 + p*BK + r; one scratch slot per beam (B*n2 + max_len*BK + r) for its current MASK row,
overwritten every step and never part of a history.  Slot table: int32 [BK, n2 + max_len + 1], beam r's row = its prefix slots,
its text history, then the MASK scratch slot; the y row of beam r uses the first n2 + t entries, the MASK row n2 + t + 1.
"""
from __future__ import annotations

import torch

from . import hip_ops as ops
from ._lib import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, MV_F32
from .beam import BeamSearch, reorder_slot_table

PAD_ID = 0
NGRAM_MIN, NGRAM_MAX = 2, 8          # mv_ngram_ban's range of n
NGRAM_MAX_IGNORE = 256               # ... of ignore ids
NGRAM_MAX_LEN = 1024                 # ... of words per history


class Generator:
    """Decode state of one engine: caches and step buffers sized for (B, N, beam, max_len); rebuilt when a call needs more."""

    def __init__(self, engine):
        self.eng = engine
        self.key = None
        self.bufs = {}
        self.ngram = 0                               # n-gram blocking: off until ngram_on(); _alloc switches it off again

    # ------------------------------------------------------------------ buffers
    def _buf(self, name, shape, dtype):
        t = self.bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.bufs[name] = torch.empty(shape, dtype=dtype, device=self.eng.device)
        return t

    def _alloc(self, B, N, K, max_len):
        eng, cfg = self.eng, self.eng.cfg
        H = cfg.hidden
        n2, BK = N + 2, B * K
        key = (B, N, K, max_len, eng.fadt)
        self.B, self.N, self.K, self.n2, self.BK, self.max_len = B, N, K, n2, BK, max_len
        self.text_base = B * n2
        self.mask_base = B * n2 + max_len * BK
        n_slots = self.mask_base + BK
        if key != self.key:
            self.kv = [torch.empty((n_slots, 2 * H), dtype=eng.fadt, device=eng.device) for _ in range(cfg.layers)]
            self.key = key
        dev = eng.device
        r = torch.arange(BK, device=dev, dtype=torch.int32)
        tbl = self._buf("tbl", (BK, n2 + max_len + 1), torch.int32)
        tbl.zero_()
        tbl[:, :n2] = (r // K).unsqueeze(1) * n2 + torch.arange(n2, device=dev, dtype=torch.int32).unsqueeze(0)
        self.tbl = tbl
        self.beam_ar = r
        self.slot_row2 = torch.cat([r, r])
        self.mslot = self.mask_base + r
        self.ws = self._buf("ws", (16 * 2 * BK * cfg.heads * (H // cfg.heads + 2),), torch.float32)
        self.ngram = 0

    def ngram_on(self, n, ignore_ids):
        """n-gram blocking for this call: two word histories per beam, used in alternation, and the ban list the next
        step's top-k reads.  The upload of the ignore ids is the only host-to-device copy blocking adds."""
        BK, max_len = self.BK, self.max_len
        self.ngram = int(n)
        self.hist = [self._buf(f"hist{i}", (BK, max_len), torch.int32) for i in range(2)]
        self.ban = self._buf("ban", (BK, max_len), torch.int32)
        self.nban = self._buf("nban", (BK,), torch.int32)
        self.nban.zero_()                            # no ban exists before n words have been produced
        self.ignore = torch.tensor(ignore_ids, dtype=torch.int32).to(self.eng.device) if ignore_ids else None

    def ngram_update(self, t, parents, y):
        """After step t's beams are chosen: every beam's history becomes its parent's plus its word, and its ban list is rebuilt."""
        ops.ngram_ban(self.hist[t & 1], self.hist[(t + 1) & 1], y, t, self.ngram, self.ban, self.nban,
                      parent=parents if t > 0 else None, ignore=self.ignore, R=self.BK)

    # ------------------------------------------------------------------ prefill
    def prefill(self, cls_tok, feats, pos, sep_tok, mask_id):
        """The prefix's K / V of every layer into its slots: the engine's forward over [CLS] + regions + [SEP] + one text row under the
        s2s mask (the prefix rows do not see the text row), keeping the per-layer projections."""
        eng, cfg = self.eng, self.eng.cfg
        B, n2, H = self.B, self.n2, cfg.hidden
        dev = eng.device
        Lp = n2 + 1
        m = torch.zeros((B, Lp, Lp), dtype=torch.int64, device=dev)
        m[:, :, :n2] = 1
        m[:, n2, n2] = 1
        txt = torch.full((B, 1), int(mask_id), dtype=torch.int64, device=dev)
        seg = torch.ones((B, 1), dtype=torch.int64, device=dev)
        eng.encoder_forward(cls_tok, txt, m, seg, feats, pos, sep_tok)
        i = torch.arange(B * Lp, device=dev, dtype=torch.int32)
        b, j = i // Lp, i % Lp
        rows = torch.where(j < n2, b * n2 + j, torch.full_like(i, -1))
        for l in range(cfg.layers):
            qkv = eng._buf(f"qkv{l}", (B * Lp, 3 * H), eng.fadt)
            ops.scatter_rows(qkv[:, H:], 3 * H, rows, B * Lp, 2 * H, self.kv[l], 2 * H)

    # ------------------------------------------------------------------ one decode step
    def _linear(self, x, name_w, bias, out, M, N, K, epi, r=None, c2=None, ldc=None):
        eng = self.eng
        W = eng.wf[name_w] if isinstance(name_w, str) else name_w
        if eng.fdt == MV_F32:
            ops.gemm(x, W, out, M=M, N=N, K=K, bias=bias, epi=epi, r=r, c2=c2, ldc=ldc)
        else:
            for m0 in range(0, M, 256):             # mv_gemm_rows takes up to 256 rows (B*K = 64 beams feed 128 + 128 rows per step)
                m1 = min(M, m0 + 256)
                ops.gemm_rows(x[m0:m1], W, out[m0:m1], M=m1 - m0, N=N, K=K, bias=bias, epi=epi, r=None if r is None else r[m0:m1], ldc=ldc)
        return out

    def step(self, t, y_prev, mask_id, k, eos_pen):
        """Rows [y_{t-1} of every beam (t > 0) | MASK of every beam] through the encoder with the cache; top-k of the MASK rows' log-probs.
        -> (vals [BK,k], idx [BK,k], logits [BK, Vp] f32)."""
        eng, cfg = self.eng, self.eng.cfg
        H, A, I, V = cfg.hidden, cfg.heads, cfg.intermediate, cfg.vocab_size
        dh = H // A
        BK, n2, dev = self.BK, self.n2, eng.device
        fadt, f32 = eng.fadt, torch.float32
        i64 = torch.int64
        mask_ids = torch.full((BK,), int(mask_id), dtype=i64, device=dev)
        if t == 0:
            R = BK
            ids = mask_ids
            pos = torch.zeros(BK, dtype=i64, device=dev)
            nk = torch.full((BK,), n2 + 1, dtype=torch.int32, device=dev)
            slot_row = self.beam_ar
            dst = self.mslot
        else:
            R = 2 * BK
            self.tbl[:, n2 + t - 1] = self.text_base + (t - 1) * BK + self.beam_ar
            ids = torch.cat([y_prev.to(i64).view(-1), mask_ids])
            pos = torch.cat([torch.full((BK,), t - 1, dtype=i64, device=dev), torch.full((BK,), t, dtype=i64, device=dev)])
            nk = torch.cat([torch.full((BK,), n2 + t, dtype=torch.int32, device=dev),
                            torch.full((BK,), n2 + t + 1, dtype=torch.int32, device=dev)])
            slot_row = self.slot_row2
            dst = torch.cat([self.text_base + (t - 1) * BK + self.beam_ar, self.mslot])
        self.tbl[:, n2 + t] = self.mslot
        seg = torch.ones(R, dtype=i64, device=dev)
        e = "enc.txt_embeddings."
        x = self._buf(f"x{R}", (R, H), fadt)
        ops.embed_rows(ids, pos, seg, eng.wf[e + "word_embeddings.weight"], eng.wf[e + "position_embeddings.weight"],
                       eng.wf[e + "token_type_embeddings.weight"], eng.p[e + "LayerNorm.weight"], eng.p[e + "LayerNorm.bias"], x,
                       R=R, H=H, V=V, maxpos=cfg.max_pos, eps=cfg.ln_eps)
        qkv = self._buf(f"qkv{R}", (R, 3 * H), fadt)
        ctx = self._buf(f"ctx{R}", (R, H), fadt)
        pre = self._buf(f"pre{R}", (R, H), f32)
        a = self._buf(f"a{R}", (R, H), fadt)
        act = self._buf(f"i{R}", (R, I), fadt)
        z = self._buf(f"z{R}", (R, I), fadt) if eng.fdt == MV_F32 else None
        mean, rstd = self._buf(f"mean{R}", (R,), f32), self._buf(f"rstd{R}", (R,), f32)
        max_nk = n2 + t + 1
        for l in range(cfg.layers):
            p = f"enc.encoder.layer.{l}."
            Wqkv, bqkv, _, _ = eng.qkv_views(l, fwd=True)
            self._linear(x, Wqkv, bqkv, qkv, R, 3 * H, H, EPI_BIAS)
            ops.scatter_rows(qkv[:, H:], 3 * H, dst, R, 2 * H, self.kv[l], 2 * H)
            kv = self.kv[l]
            ops.attn_decode(qkv, kv, kv[:, H:], self.tbl, nk, ctx, R=R, A=A, dh=dh, max_nk=max_nk, ldq=3 * H, ldkv=2 * H,
                            slot_row=slot_row, nsplit=0, ws=self.ws)
            self._linear(ctx, p + "attention.output.dense.weight", eng.p[p + "attention.output.dense.bias"], pre, R, H, H, EPI_BIAS_RES, r=x)
            ops.layernorm_fwd(pre, eng.p[p + "attention.output.LayerNorm.weight"], eng.p[p + "attention.output.LayerNorm.bias"], a, mean,
                              rstd, R, H, cfg.ln_eps)
            self._linear(a, p + "intermediate.dense.weight", eng.p[p + "intermediate.dense.bias"], act, R, I, H, EPI_BIAS_GELU, c2=z)
            self._linear(act, p + "output.dense.weight", eng.p[p + "output.dense.bias"], pre, R, H, I, EPI_BIAS_RES, r=a)
            ops.layernorm_fwd(pre, eng.p[p + "output.LayerNorm.weight"], eng.p[p + "output.LayerNorm.bias"], x, mean, rstd, R, H,
                              cfg.ln_eps)
        # MLM head on the MASK rows (the last BK rows): transform (dense + GELU + LayerNorm eps 1e-5), tied decoder
        xm = x[R - BK:]
        tact = self._buf("tact", (BK, H), f32)
        tz = self._buf("tz", (BK, H), f32) if eng.fdt == MV_F32 else None
        self._linear(xm, "mlm.predictions.transform.dense.weight", eng.p["mlm.predictions.transform.dense.bias"], tact, BK, H, H,
                     EPI_BIAS_GELU, c2=tz)
        tt = self._buf("t", (BK, H), fadt)
        ops.layernorm_fwd(tact, eng.p["mlm.predictions.transform.LayerNorm.weight"], eng.p["mlm.predictions.transform.LayerNorm.bias"], tt,
                          mean[:BK], rstd[:BK], BK, H, cfg.head_ln_eps)
        Vp = (V + 7) // 8 * 8
        logits = self._buf("logits", (BK, Vp), f32)
        self._linear(tt, "enc.txt_embeddings.word_embeddings.weight", eng.p["mlm.predictions.bias"], logits, BK, V, H, EPI_BIAS, ldc=Vp)
        if self.ngram:
            vals, idx = ops.logprob_topk_banned(logits, k, R=BK, V=V, ld=Vp, eos_penalty_id=eos_pen, ban=self.ban, nban=self.nban)
        else:
            vals, idx = ops.logprob_topk(logits, k, R=BK, V=V, ld=Vp, eos_penalty_id=eos_pen)
        return vals, idx, logits[:, :V]


@torch.no_grad()
def generate(model, cls_tok, input_img, sep_tok, max_len=254, beam_size=1, min_len=0, length_penalty=0.0, eos_id=102, mask_id=103,
             forced_ids=None, return_traces=False, forbid_duplicate_ngrams=False, forbid_ignore_set=None, no_repeat_ngram_size=0,
             no_repeat_ignore_ids=None):
    """See CXRBERT.generate.

    n-gram blocking: the reference's `forbid_duplicate_ngrams=True, ngram_size=n, forbid_ignore_set=S` is spelled
    `no_repeat_ngram_size=n, no_repeat_ignore_ids=S` here (n in 2..8, S an iterable of token ids, at most 256); the reference's own
    keyword names are refused.  With blocking on, beam_size=1 runs the beam search at K = 1 (the reference's beam_search, which is
    where its rule lives; its separate greedy loop ignores the flags) and returns what a beam call returns."""
    if forbid_duplicate_ngrams or forbid_ignore_set:
        raise NotImplementedError("forbid_duplicate_ngrams / ngram_size / forbid_ignore_set are spelled no_repeat_ngram_size=n / "
                                  "no_repeat_ignore_ids=S here")
    ngram = int(no_repeat_ngram_size or 0)
    ignore_ids = sorted({int(i) for i in no_repeat_ignore_ids}) if no_repeat_ignore_ids is not None else []
    if ngram:
        if not NGRAM_MIN <= ngram <= NGRAM_MAX:
            raise ValueError(f"no_repeat_ngram_size must be 0 (off) or in {NGRAM_MIN}..{NGRAM_MAX}")
        if forced_ids is not None:
            raise ValueError("forced_ids (teacher-forced scoring) cannot be combined with no_repeat_ngram_size")
        if len(ignore_ids) > NGRAM_MAX_IGNORE:
            raise ValueError(f"no_repeat_ignore_ids holds more than {NGRAM_MAX_IGNORE} ids")
    eng, cfg = model.engine, model.cfg
    if eng.device.type != "cuda":
        raise RuntimeError("medvill HIP kernels need CUDA(ROCm) tensors; there is no CPU fallback")
    K = int(beam_size)
    if not 1 <= K <= 16:
        raise ValueError("beam_size must be in 1..16")
    if forced_ids is not None:
        if K != 1:
            raise ValueError("forced_ids (teacher-forced scoring) needs beam_size=1")
        forced_ids = forced_ids.to(eng.device, torch.int64)
        max_len = int(forced_ids.shape[1])
    max_len = int(max_len)
    if not 1 <= max_len <= cfg.max_pos:
        raise ValueError(f"max_len must be in 1..max_position_embeddings ({cfg.max_pos})")
    if ngram and max_len > NGRAM_MAX_LEN:
        raise ValueError(f"no_repeat_ngram_size needs max_len <= {NGRAM_MAX_LEN}")
    feats, pos = model._regions(input_img)
    B, N = int(feats.shape[0]), int(feats.shape[1])
    if forced_ids is not None and forced_ids.shape[0] != B:
        raise ValueError("forced_ids must be [B, T]")
    if model._params_dirty():
        eng.shadow_dirty = True
    gen = model.__dict__.get("_generator")
    if gen is None or gen.eng is not eng:
        gen = model.__dict__["_generator"] = Generator(eng)
    prev = (eng.training, eng.keep_acts, eng.drop_counter)
    eng.training, eng.keep_acts = False, True           # eval mode; the prefill keeps its per-layer projections
    try:
        gen._alloc(B, N, K, max_len)
        gen.prefill(cls_tok, feats, pos, sep_tok, mask_id)
        eng.keep_acts = prev[1]
        dev = eng.device
        if ngram:
            gen.ngram_on(ngram, ignore_ids)
        if K == 1 and not ngram:
            ids = torch.full((B, max_len), PAD_ID, dtype=torch.int64, device=dev)
            logp = torch.zeros((B, max_len), dtype=torch.float32, device=dev)
            step_logits = torch.empty((B, max_len, cfg.vocab_size), dtype=torch.float32, device=dev) if forced_ids is not None else None
            done = torch.zeros(B, dtype=torch.bool, device=dev)
            y = None
            for t in range(max_len):
                vals, idx, logits = gen.step(t, y, mask_id, 1, eos_id if t < min_len else -1)
                yt, lt = idx[:, 0], vals[:, 0]
                if forced_ids is not None:
                    step_logits[:, t] = logits
                    lt = torch.log_softmax(logits, dim=-1).gather(1, forced_ids[:, t:t + 1]).squeeze(1)
                    ids[:, t] = yt
                    logp[:, t] = lt
                    y = forced_ids[:, t]
                    continue
                ids[:, t] = torch.where(done, torch.full_like(yt, PAD_ID), yt)
                logp[:, t] = torch.where(done, torch.zeros_like(lt), lt)
                done = done | (yt == eos_id)
                y = yt
                if (t & 7) == 7 and bool(done.all()):
                    break
            if forced_ids is not None:
                return ids, logp, step_logits
            return ids, logp
        bs = BeamSearch(B, K, eos_id, length_penalty)
        y = None
        for t in range(max_len):
            vals, idx, _ = gen.step(t, y, mask_id, K, eos_id if t < min_len else -1)
            back, k_ids = bs.step(vals, idx)
            parents = bs.parents(back)
            reorder_slot_table(gen.tbl, parents, gen.n2, gen.n2 + t)
            y = k_ids.reshape(-1)
            if ngram and t + 1 < max_len:
                gen.ngram_update(t, parents, y)
            if (t & 7) == 7 and bool(bs.all_done()):
                break
        out, scores, traces = bs.finalize(max_len, PAD_ID)
        out, scores = out.to(dev), scores.to(dev)
        if return_traces:
            return out, scores, {k_: v.to(dev) for k_, v in traces.items()}
        return out, scores
    finally:                # sticky engine state: a later training step or direct Engine user must find what it left
        # (the dropout counter too: a training step after generate() draws the masks it would have drawn without it)
        eng.training, eng.keep_acts, eng.drop_counter = prev
