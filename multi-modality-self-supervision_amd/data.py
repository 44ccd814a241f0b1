"""Batch-side contract of the pretraining path: attention-mask families, label layout and a
synthetic batch generator that produces the reference Dataset's 9-tuple contents directly on
the device (no PIL / tokenizer / DataLoader workers on the benchmark path).

Mirrors (paths relative to the upstream repo):
  mask families ............. data/dataset_origin.py:138-176  (closed forms: SURVEY Appendix B)
  label / pad / segment ..... data/dataset_origin.py:105-135
  MLM corruption ............ data/dataset_origin.py:183-209 (15 % / 80-10-10, >= 1 label)
  region sampling ........... models/image.py:63-68 (sorted sample of M positions, shared by the batch)
"""
from __future__ import annotations

import torch

PAD, UNK, CLS, SEP, MASK = 0, 100, 101, 102, 103
FAMILIES = ("full", "s2s", "bar", "noncross", "1d")


FAMILY_ID = {"full": 0, "s2s": 1, "bar": 2, "noncross": 3, "1d": 4}


class MaskDesc:
    """Per-sample mask descriptors {family, n2, vl} (int32 [B,3]): what the attention kernels need instead of the
    reference's materialised int64 [B,L,L] matrices.  Accepted wherever `attn_mask` is (CXRBERT.forward, TrainStep)."""

    def __init__(self, desc: torch.Tensor, L: int, host: torch.Tensor = None):
        self.desc, self.L = desc.to(torch.int32), int(L)
        self._host = host                # CPU copy (kept when the descriptors were built on the host: no sync later)

    def host_desc(self) -> torch.Tensor:
        if self._host is None:
            self._host = self.desc.cpu()
        return self._host

    def packable(self) -> bool:
        """True when no valid query can see a position after the text [SEP] (full / seq2seq / 1-D families)."""
        f = self.host_desc()[:, 0]
        return bool(((f == 0) | (f == 1) | (f == 4)).all())

    @classmethod
    def make(cls, family, N: int, S: int, n_ids, device="cpu"):
        """family: one name for the whole batch or a per-sample sequence of names (Mixed)."""
        n_ids = torch.as_tensor(n_ids, dtype=torch.int32).view(-1)
        B = n_ids.numel()
        fam = [family] * B if isinstance(family, str) else list(family)
        d = torch.empty((B, 3), dtype=torch.int32)
        d[:, 0] = torch.tensor([FAMILY_ID[f] for f in fam], dtype=torch.int32)
        d[:, 1] = N + 2
        d[:, 2] = N + 2 + n_ids
        return cls(d.to(device), S + N + 3, host=d)

    def dim(self):
        return 3

    def __getitem__(self, idx):          # batch slicing, like a [B, ...] tensor
        return MaskDesc(self.desc[idx].reshape(-1, 3), self.L, None if self._host is None else self._host[idx].reshape(-1, 3))

    def __len__(self):
        return int(self.desc.shape[0])

    def to(self, device, *a, **k):
        return MaskDesc(self.desc.to(device), self.L, self._host)


def descriptors_from_dense(mask: torch.Tensor, input_ids: torch.Tensor, N: int):
    """HYPOTHESIS {family, n2, vl} per sample for a materialised reference mask (dataset_origin.py:138-176), from two rows and a column
    per sample -- the torch restatement, on whatever device the tensors live on, of the trainer's host recogniser
    (CXRBERT_Trainer._recognise_masks: same probes, same precedence).  Nothing is read back: -> (desc int32 [B,3], ok bool []) with
    `ok` false when some sample matches no family; the caller confirms the hypothesis entry by entry (CXRBERT._mask_descriptors compares
    the mask words of mv_mask_pack(mask) and mv_mask_build(desc)) before anything runs on it.  None when the shapes rule it out."""
    if not torch.is_tensor(mask) or mask.dtype != torch.int64 or mask.dim() not in (2, 3):
        return None
    B, L = mask.shape[0], mask.shape[-1]
    S, n2 = L - N - 3, N + 2
    if S < 1 or tuple(input_ids.shape) != (B, S + 1):
        return None
    dev = mask.device
    ids = input_ids.to(dev)
    T = S + 1
    t = torch.arange(T, device=dev).view(1, T)
    # valid length from the LAST non-zero id (random_word, dataset_origin.py:183-209, may put id 0 at a labelled in-text position)
    last = torch.where(ids != 0, t, torch.full_like(t, -1)).max(dim=1).values
    vl = n2 + last + 1
    j = torch.arange(L, device=dev).view(1, L)
    full_row = (j < vl.view(B, 1)).to(torch.int64)
    if mask.dim() == 2:
        fam = torch.full((B,), FAMILY_ID["1d"], dtype=torch.int64, device=dev)
        ok = (mask == full_row).all()
    else:
        r0, rl, cl = mask[:, 0, :], mask[:, L - 1, :], mask[:, :, L - 1]
        img_row, txt_row = (j < n2).to(torch.int64), (j >= n2).to(torch.int64)
        bar_col = ((j < n2) | (j == L - 1)).to(torch.int64)
        eq = lambda a, b: (a == b).all(dim=1)
        one = lambda a: (a == 1).all(dim=1)
        # (the last column tells a full-length BAR sample -- whose probe ROWS are all ones too -- from a full one)
        is_full = eq(r0, full_row) & eq(rl, full_row) & eq(cl, full_row[:, L - 1:L].expand(B, L))
        is_s2s = eq(r0, img_row) & one(rl)
        is_bar = one(r0) & one(rl) & eq(cl, bar_col)
        is_non = eq(r0, img_row) & eq(rl, txt_row)
        fam = torch.full((B,), -1, dtype=torch.int64, device=dev)
        for cond, name in ((is_non, "noncross"), (is_bar, "bar"), (is_s2s, "s2s"), (is_full, "full")):     # later entries win
            fam = torch.where(cond, torch.full_like(fam, FAMILY_ID[name]), fam)
        ok = (fam >= 0).all()
    desc = torch.stack([fam.clamp(min=0), torch.full_like(fam, n2), vl], dim=1).to(torch.int32)
    return desc, ok


def build_mask(family: str, N: int, S: int, n_ids, device="cpu") -> torch.Tensor:
    """int64 [B,L,L] (or [B,L] for '1d') for per-sample text lengths n_ids (incl. the text [SEP])."""
    n_ids = torch.as_tensor(n_ids, device=device, dtype=torch.int64).view(-1)
    B = n_ids.numel()
    L = S + N + 3
    n2 = N + 2
    vl = (n2 + n_ids).view(B, 1, 1)
    i = torch.arange(L, device=device).view(1, L, 1)
    j = torch.arange(L, device=device).view(1, 1, L)
    if family == "full":
        m = (j < vl).expand(B, L, L)
    elif family == "s2s":
        m = ((j < n2) | ((i >= n2) & (j >= n2) & (j <= i))).expand(B, L, L)
    elif family == "bar":
        m = ((i < n2) | (j < n2) | (j <= i)).expand(B, L, L)
    elif family == "noncross":
        m = ((i < n2) == (j < n2)).expand(B, L, L)
    elif family == "1d":
        return (torch.arange(L, device=device).view(1, L) < vl.view(B, 1)).to(torch.int64)
    else:
        raise ValueError(family)
    return m.to(torch.int64).contiguous()


def mixed_mask(N: int, S: int, n_ids, choose_s2s, device="cpu"):
    """`Mixed` (dataset_origin.py:152-155): per-sample choice between full and s2s."""
    full = build_mask("full", N, S, n_ids, device)
    s2s = build_mask("s2s", N, S, n_ids, device)
    sel = torch.as_tensor(choose_s2s, device=device, dtype=torch.bool).view(-1, 1, 1)
    return torch.where(sel, s2s, full)


def assemble_batch(ids: torch.Tensor, lengths: torch.Tensor, N: int, vocab: int, key: int, family="full", draws=None) -> dict:
    """Device-side sample assembly from RAW token ids (HIP kernels mv_mlm_draws / mv_mlm_corrupt): the MLM corruption
    of random_word (dataset_origin.py:183-209), [SEP]/[PAD]/label/segment layout (:105-135), mask descriptors and the
    labelled-row index.  ids int64 [B,S] on the GPU, valid for t < lengths[b].  `draws` = (u f32 [B,S], rnd int32 [B,S])
    overrides the hash-generated random sources.  One host sync (the label count)."""
    from . import hip_ops as ops
    B, S = ids.shape
    dev = ids.device
    u, rnd = draws if draws is not None else ops.mlm_draws(key, B, S, vocab, dev)
    fams = [family] * B if isinstance(family, str) else list(family)
    fam_t = torch.tensor([FAMILY_ID[f] for f in fams], dtype=torch.int32).to(dev)
    out = ops.mlm_corrupt(ids, lengths.to(torch.int32), u, rnd, N, family=fam_t)
    n = int(out["n_labels"].item())
    return dict(input_txt=out["input_txt"], segment=out["segment"], txt_labels=out["txt_labels"], n_ids=out["n_ids"].to(torch.int64),
                label_rows=out["label_rows"][:n], label_ids=out["label_ids"][:n], attn_desc=MaskDesc(out["desc"], S + N + 3))


def corrupt_tokens(ids: torch.Tensor, lengths: torch.Tensor, vocab: int, gen: torch.Generator):
    """Host-side (torch) vectorised random_word for CPU-only tooling and tests; the GPU path is `assemble_batch`.
    ids [B,S] (valid for t < lengths[b]).  Returns (ids', labels) with labels = original id where selected
    else -100; guarantees >= 1 label per sample."""
    B, S = ids.shape
    dev = ids.device
    t = torch.arange(S, device=dev).view(1, S)
    valid = t < lengths.view(B, 1)
    u = torch.rand((B, S), generator=gen, device=dev)
    sel = (u < 0.15) & valid
    none = ~sel.any(dim=1)
    sel[none, 0] = True                       # "at least one mask": position 0 becomes [MASK]
    u2 = u / 0.15
    rnd = torch.randint(0, vocab, (B, S), generator=gen, device=dev)
    out = ids.clone()
    to_mask = sel & ((u2 < 0.8) | none.view(B, 1))
    to_rand = sel & (u2 >= 0.8) & (u2 < 0.9) & ~none.view(B, 1)
    out[to_mask] = MASK
    out[to_rand] = rnd[to_rand]
    labels = torch.where(sel, ids, torch.full_like(ids, -100))
    return out, labels


def synthetic_batch(vocab: int, B: int, N: int, S: int, family: str, seed: int, device="cuda", img_hidden: int = 2048,
                    M_regions: int = 256, feat_dtype=torch.float32, lengths=None) -> dict:
    """One mini-batch in the reference's batch protocol (dataset_origin.py:181) plus the
    labelled-row index the fused MLM head consumes.  family: full|s2s|bar|noncross|1d|mixed."""
    dev = torch.device(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    T, L = S + 1, S + N + 3
    lo = 1000 if vocab > 2000 else 200
    drawn = torch.randint((S + 1) // 2, S + 1, (B,), generator=gen, device=dev)      # len ~ U{ceil(S/2)..S}
    lengths = drawn if lengths is None else torch.as_tensor(lengths, dtype=torch.int64).clamp(1, S).to(dev)
    ids = torch.randint(lo, vocab, (B, S), generator=gen, device=dev)
    n_ids = lengths + 1
    if dev.type == "cuda":
        asm = assemble_batch(ids, lengths, N, vocab, key=0x5EED0000 + seed)     # family descriptors are filled in below
        txt, labels, segment = asm["input_txt"], asm["txt_labels"], asm["segment"]
        rows, lids = asm["label_rows"], asm["label_ids"]
    else:
        ids_c, lab = corrupt_tokens(ids, lengths, vocab, gen)
        t = torch.arange(T, device=dev).view(1, T)
        txt = torch.zeros((B, T), dtype=torch.int64, device=dev)
        txt[:, :S] = torch.where(t[:, :S] < lengths.view(B, 1), ids_c, torch.zeros_like(ids_c))
        txt[torch.arange(B, device=dev), lengths] = SEP
        labels = torch.full((B, L), -100, dtype=torch.int64, device=dev)
        labels[:, N + 2:N + 2 + S] = torch.where(t[:, :S] < lengths.view(B, 1), lab, torch.full_like(lab, -100))
        segment = torch.ones((B, T), dtype=torch.int64, device=dev)
        rows, lids = label_index(labels)
    perm = torch.randperm(M_regions, generator=gen, device=dev)[:N]
    pos = torch.sort(perm)[0].view(1, N).expand(B, N).contiguous()
    feats = torch.randn((B, N, img_hidden), generator=gen, device=dev, dtype=torch.float32).to(feat_dtype)
    is_aligned = (torch.rand((B,), generator=gen, device=dev) > 0.5).to(torch.int64)
    if family == "mixed":
        choose = torch.rand((B,), generator=gen, device=dev) < 0.75
        mask = mixed_mask(N, S, n_ids, choose, dev)
        fams = ["s2s" if c else "full" for c in choose.tolist()]
    else:
        mask = build_mask(family, N, S, n_ids, dev)
        fams = family
    desc = MaskDesc.make(fams, N, S, n_ids.cpu(), dev)
    return dict(cls_tok=torch.full((B, 1), CLS, dtype=torch.int64, device=dev), input_txt=txt, attn_mask=mask, segment=segment,
                img_feats=feats, img_pos=pos, sep_tok=torch.full((B, 1), SEP, dtype=torch.int64, device=dev), txt_labels=labels,
                is_aligned=is_aligned, n_ids=n_ids, label_rows=rows, label_ids=lids, attn_desc=desc)


def label_index(txt_labels: torch.Tensor):
    """(rows int32 [R], ids int32 [R]) of the positions with a label (!= -100), row-major."""
    flat = txt_labels.reshape(-1)
    rows = torch.nonzero(flat != -100).view(-1)
    return rows.to(torch.int32), flat[rows].to(torch.int32)


_S2S_FAMILY = {"s2s": "s2s", "bi": "1d", "bar": "bar"}


def seq2seq_finetune_batch(ids, lengths, n_regions: int, max_len: int, max_pred: int = 10, mask_prob: float = 0.15, mode: str = "s2s",
                           generator: torch.Generator = None) -> dict:
    """Host-side batch of the report fine-tuning task as Preprocess4Seq2seq lays it out (Downstream_task/report_generation_and_vqa/sc/
    data_loader.py:340-419): the inputs of CXRBertForReportFinetune.forward except the image.
      ids int64 [B, >= max(lengths)] raw text token ids, valid for t < lengths[b]; max_len = the full sequence length
      [CLS] + n_regions + [SEP] + text, so the text part holds T = max_len - n_regions - 2 ids including its final [SEP].
      n_pred = min(max_pred, max(1, int(round(len * mask_prob)))) (Python's round); candidates are all text positions including the
      last [SEP]; with probability 1/2 the last [SEP] takes the final slot (so it can be listed twice); masked positions hold [MASK];
      the lists are padded with position 0, label 0, weight 0.  mode "s2s" / "bi" / "bar": data_loader.py:395-412 -> the s2s, 1-D and
      BAR mask families (a MaskDesc).  Seeded by `generator` alone; no claim of bit-equality with random.shuffle."""
    if mode not in _S2S_FAMILY:
        raise ValueError(f"mode {mode!r}: one of {sorted(_S2S_FAMILY)}")
    ids = torch.as_tensor(ids).detach().cpu().to(torch.int64)
    lengths = torch.as_tensor(lengths).detach().cpu().to(torch.int64).view(-1)
    B, N = int(lengths.numel()), int(n_regions)
    T = int(max_len) - N - 2
    if T < 2 or int(lengths.min()) < 1 or int(lengths.max()) > T - 1 or ids.shape[0] != B or ids.shape[1] < int(lengths.max()):
        raise ValueError(f"text lengths must lie in [1, {T - 1}] (max_len {max_len} = [CLS] + {N} regions + [SEP] + text + [SEP])")
    gen = generator if generator is not None else torch.Generator().manual_seed(torch.initial_seed())
    txt = torch.zeros((B, T), dtype=torch.int64)
    segment = torch.zeros((B, T), dtype=torch.int64)
    pos = torch.zeros((B, max_pred), dtype=torch.int64)
    lab = torch.zeros((B, max_pred), dtype=torch.int64)
    w = torch.zeros((B, max_pred), dtype=torch.float32)
    for b in range(B):
        n = int(lengths[b])
        txt[b, :n] = ids[b, :n]
        txt[b, n] = SEP
        segment[b, :n + 1] = 1
        n_pred = min(max_pred, max(1, int(round(n * mask_prob))))
        cand = torch.randperm(n + 1, generator=gen)                   # text indices 0 .. n (n: the last [SEP])
        if float(torch.rand(1, generator=gen)) > 0.5:
            chosen = cand[:n_pred - 1].tolist() + [n]
        else:
            chosen = cand[:n_pred].tolist()
        for j, t in enumerate(chosen):
            pos[b, j], lab[b, j], w[b, j] = N + 2 + t, ids[b, t] if t < n else SEP, 1.0
        txt[b, chosen] = MASK
    n_ids = lengths + 1
    return dict(cls_tok=torch.full((B, 1), CLS, dtype=torch.int64), input_txt=txt, segment=segment,
                sep_tok=torch.full((B, 1), SEP, dtype=torch.int64), attn_mask=MaskDesc.make(_S2S_FAMILY[mode], N, T - 1, n_ids),
                masked_pos=pos, masked_lm_labels=lab, masked_weights=w, n_ids=n_ids)


# ---------------------------------------------------------------------------------------------------- device-resident banks
def check_pairs(pairs, n_images: int, n_texts: int) -> torch.Tensor:
    """Host-side check of a pair list given on the host: -> int32 [R, 2] (image item, text item), every index inside its bank."""
    p = torch.as_tensor(pairs)
    if p.dim() != 2 or p.shape[1] != 2 or p.shape[0] == 0 or p.dtype.is_floating_point or p.dtype == torch.bool:
        raise ValueError("pairs must be a non-empty integer [R, 2] list of (image item, text item)")
    p = p.to(torch.int64)
    if int(p[:, 0].min()) < 0 or int(p[:, 0].max()) >= n_images:
        raise IndexError(f"pairs name an image outside the bank of {n_images}")
    if int(p[:, 1].min()) < 0 or int(p[:, 1].max()) >= n_texts:
        raise IndexError(f"pairs name a text outside the bank of {n_texts}")
    return p.to(torch.int32).contiguous()


class DeviceBank:
    """What the device-resident banks share: a text side and an image side filled once, and the host half of a batch -- the index
    list, the mask family per sample and the descriptors' host copy -- so that no batch reads anything back.
      add_texts(ids, lengths)   ids int64 [n, S+1], each row tokens + [SEP] + [PAD]... as data_processing
                                (Downstream_task/Retrieval/full_dset_retrieval.py:183-198) lays it out; lengths [n] count the [SEP]
      add_images(input_img)     whatever CXRBERT.forward accepts as input_img -- (region features [n, N, F], positions [n, N]) or pixels for
                                the model's region encoder -- run ONCE per distinct image; the features are stored in the engine's input
                                encoding
    `model`: a task model or a CXRBERT (its engine gives device and encoding); None with device= / feat_dtype= for host-only use."""

    def __init__(self, model=None, device=None, feat_dtype=None):
        bert = getattr(model, "bert", model)
        self.bert = bert
        if bert is not None:
            eng = bert.engine
            device = eng.device if device is None else device
            feat_dtype = (eng.adt if eng.is16 else torch.float32) if feat_dtype is None else feat_dtype
        self.device = torch.device(device if device is not None else "cpu")
        self.feat_dtype = feat_dtype if feat_dtype is not None else torch.float32
        self.txt_ids = self.txt_len = self.img_feats = self.img_pos = None
        self._len_host = None
        self._tok = {}

    @property
    def n_texts(self):
        return 0 if self.txt_ids is None else int(self.txt_ids.shape[0])

    @property
    def n_images(self):
        return 0 if self.img_feats is None else int(self.img_feats.shape[0])

    def add_texts(self, ids, lengths):
        ids = torch.as_tensor(ids).to(torch.int64)
        lens = torch.as_tensor(lengths).to(torch.int32).reshape(-1)
        if ids.dim() != 2 or ids.shape[1] < 2 or lens.numel() != ids.shape[0]:
            raise ValueError("add_texts: ids int64 [n, S+1] and one length per row")
        host = lens.cpu()               # (one copy when the bank is filled: batches never read lengths back)
        if int(host.min()) < 1 or int(host.max()) > ids.shape[1]:
            raise ValueError(f"add_texts: lengths count the [SEP], so they lie in [1, {ids.shape[1]}]")
        if self.txt_ids is not None and self.txt_ids.shape[1] != ids.shape[1]:
            raise ValueError("add_texts: every row of the bank has the same S+1 columns")
        ids, lens = ids.to(self.device).contiguous(), lens.to(self.device).contiguous()
        self.txt_ids = ids if self.txt_ids is None else torch.cat([self.txt_ids, ids])
        self.txt_len = lens if self.txt_len is None else torch.cat([self.txt_len, lens])
        self._len_host = host if self._len_host is None else torch.cat([self._len_host, host])
        return self

    @torch.no_grad()
    def add_images(self, input_img):
        if self.bert is not None:
            feats, pos = self.bert._regions(input_img)
        else:
            feats, pos = input_img
        if feats.dim() != 3 or tuple(pos.shape) != tuple(feats.shape[:2]):
            raise ValueError("add_images: region features [n, N, F] and positions [n, N]")
        if self.img_feats is not None and tuple(self.img_feats.shape[1:]) != tuple(feats.shape[1:]):
            raise ValueError("add_images: every image of the bank has the same [N, F] regions")
        feats = feats.detach().to(self.device, self.feat_dtype).contiguous()
        pos = pos.detach().to(self.device, torch.int64).contiguous()
        self.img_feats = feats if self.img_feats is None else torch.cat([self.img_feats, feats])
        self.img_pos = pos if self.img_pos is None else torch.cat([self.img_pos, pos])
        return self

    def _tokens(self, R):
        t = self._tok.get(R)
        if t is None:
            t = self._tok[R] = (torch.full((R, 1), CLS, dtype=torch.int64, device=self.device),
                                torch.full((R, 1), SEP, dtype=torch.int64, device=self.device))
        return t

    @staticmethod
    def _index_list(idx, bound: int, noun: str) -> torch.Tensor:
        """An index list given on the host, checked against the bank of `bound` `noun`: -> int64 [B]."""
        h = torch.as_tensor(idx).reshape(-1)
        if h.numel() == 0 or h.dtype.is_floating_point or h.dtype == torch.bool:
            raise ValueError(f"idx must be a non-empty integer list of {noun}")
        h = h.to(torch.int64)
        if int(h.min()) < 0 or int(h.max()) >= bound:
            raise IndexError(f"idx outside the bank of {bound} {noun}")
        return h

    def _indices(self, idx, bound: int, noun: str):
        """A batch's index list -> (int32 [B] on the device, int64 [B] on the host or None).  A device tensor is taken as it is (the
        kernel clamps it into the bank); anything else passes _index_list."""
        if torch.is_tensor(idx) and idx.device.type != "cpu":
            if idx.dtype != torch.int32 or idx.dim() != 1:
                raise TypeError("idx on the device: int32 [B]")
            return idx.contiguous(), None
        h = self._index_list(idx, bound, noun)
        return h.to(torch.int32).to(self.device), h

    @staticmethod
    def _families(mode, B: int) -> torch.Tensor:
        """mode "s2s" / "bi" / "bar", or one per sample -> the mask family of each sample, int32 [B] on the host."""
        modes = [mode] * B if isinstance(mode, str) else list(mode)
        if len(modes) != B or any(m not in _S2S_FAMILY for m in modes):
            raise ValueError(f"mode: one of {sorted(_S2S_FAMILY)}, or one per sample ({B})")
        return torch.tensor([FAMILY_ID[_S2S_FAMILY[m]] for m in modes], dtype=torch.int32)

    def host_descriptors(self, text_items, family):
        """int32 [B, 3] = {family, N+2, N+2+len}: what an assemble kernel writes, from the host copy of the lengths.  text_items int64 [B]
        on the host; family: one id, or int32 [B]."""
        N = int(self.img_feats.shape[1])
        d = torch.empty((text_items.numel(), 3), dtype=torch.int32)
        d[:, 0], d[:, 1], d[:, 2] = family, N + 2, N + 2 + self._len_host.index_select(0, text_items)
        return d

    def _batch(self, out, host_desc):
        """The six arguments every task's forward starts with, from an assemble kernel's outputs: (cls_tok, input_txt, attn_mask,
        segment, input_img, sep_tok), attn_mask a MaskDesc, input_img = (features, positions)."""
        B, (N, T) = int(out["desc"].shape[0]), (int(self.img_feats.shape[1]), int(self.txt_ids.shape[1]))
        cls_tok, sep_tok = self._tokens(B)
        return cls_tok, out["input_txt"], MaskDesc(out["desc"], T + N + 2, host=host_desc), out["segment"], (out["feats"], out["pos"]), sep_tok


# ---------------------------------------------------------------------------------------------------- retrieval banks
class RetrievalBank(DeviceBank):
    """The two sides of a retrieval data set, resident on the device (Downstream_task/Retrieval/full_dset_retrieval.py builds every pair
    on the host, and pushes an image through the region encoder once per pair it appears in):
      add_texts, add_images     DeviceBank's
      set_classes(class_id)     the class of every item, for the sampler's label_conditioned mode
      assemble(pairs)           (image item, text item) index pairs -> the arguments of CXRBertForRetrieval.forward, with `attn_mask` a
                                MaskDesc of the 1-D family (one mv_pair_assemble launch).  Pairs given on the host are checked against the
                                banks there and the descriptors' host copy is built from the lengths' host copy (no read-back); pairs that
                                live on the device are clamped into the banks by the kernel."""

    def __init__(self, model=None, device=None, feat_dtype=None, class_id=None):
        super().__init__(model, device, feat_dtype)
        self.set_classes(class_id)

    def set_classes(self, class_id):
        """int [n]: the class of item i for the sampler's label_conditioned mode (None: plain sampling)."""
        self.class_id = None if class_id is None else torch.as_tensor(class_id).to(torch.int32).reshape(-1).to(self.device).contiguous()
        return self

    def host_descriptors(self, pairs_host):
        """int32 [R, 3] = {FAMILY_ID['1d'], N+2, N+2+len}: what mv_pair_assemble writes, from the host copy of the lengths."""
        return super().host_descriptors(pairs_host[:, 1].to(torch.int64), FAMILY_ID["1d"])

    def assemble(self, pairs):
        """-> (cls_tok, input_txt, attn_mask, segment, input_img, sep_tok), attn_mask a MaskDesc, input_img = (features, positions)."""
        from . import hip_ops as ops
        if self.txt_ids is None or self.img_feats is None:
            raise RuntimeError("RetrievalBank.assemble: fill both banks first (add_texts, add_images)")
        host = None
        if torch.is_tensor(pairs) and pairs.device.type != "cpu":
            if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
                raise TypeError("pairs on the device: int32 [R, 2]")
            dev_pairs = pairs.contiguous()
        else:
            hp = check_pairs(pairs, self.n_images, self.n_texts)
            host = self.host_descriptors(hp)
            dev_pairs = hp.to(self.device)
        return self._batch(ops.pair_assemble(self.txt_ids, self.txt_len, self.img_feats, self.img_pos, dev_pairs), host)


# ---------------------------------------------------------------------------------------------------- report bank
class ReportBank(DeviceBank):
    """A report-generation data set resident on the device, item i = (image i, report i): what seq2seq_finetune_batch builds per sample on
    the host (Preprocess4Seq2seq, Downstream_task/report_generation_and_vqa/sc/data_loader.py:330-419) comes out of one
    mv_report_assemble launch per batch, and an image passes the region encoder once, not once per epoch.
      add_reports(ids, lengths)  ids int64 [n, T], each row tokens + [SEP] + [PAD]... (DeviceBank.add_texts' layout); lengths [n] count
                                 the [SEP].  Also fixes n_pred = min(max_pred, max(1, int(round((len - 1) * mask_prob)))) per item, with
                                 Python's round as in the reference (1.5 -> 2, 4.5 -> 4), from the host copy of the lengths.
      add_images(input_img)      as DeviceBank.add_images
      assemble(idx, mode, ...)   -> (cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, lists): the arguments of
                                 CXRBertForReportFinetune.forward and lists = dict(masked_lm_labels, masked_pos, masked_weights) on the
                                 device.  mode "s2s" / "bi" / "bar" (data_loader.py:395-412) or one per sample -- the reference draws the
                                 pipeline per sample with random.choices (:282); that draw stays with the caller.  (key, step) select the
                                 masking draw's random words; `draws` [B, T+1] overrides them (hip_ops.report_assemble).  idx given on the
                                 host is checked against the bank there and the descriptors' host copy comes from the host lengths and
                                 modes (no read-back); idx on the device (int32) is clamped into the bank by the kernel.
      set_vocab(tokens), set_references(texts=None)
                                 what model.evaluate (report_eval.evaluate: corpus BLEU-1..4 of the generated reports) needs: the word
                                 tables of the vocabulary and every item's reference words as 64-bit keys on the device."""

    def __init__(self, model=None, device=None, feat_dtype=None, max_pred=10, mask_prob=0.15):
        super().__init__(model, device, feat_dtype)
        self.max_pred, self.mask_prob = int(max_pred), float(mask_prob)
        if self.max_pred < 1:
            raise ValueError("ReportBank: max_pred >= 1")
        self.n_pred = None
        self.vocab = self.ref_key = self.ref_n = None

    def set_vocab(self, tokens):
        """The vocabulary, id -> token string, for the BLEU evaluation: report_eval.word_tables' tables go onto the device; the ids of
        '[SEP]' and '[PAD]', at which a generated row ends, are looked up by name as the reference does."""
        from .report_eval import END_TOKENS, word_tables
        tokens = list(tokens)
        missing = [t for t in END_TOKENS if t not in tokens]
        if missing:
            raise ValueError(f"set_vocab: the vocabulary has no {' / '.join(missing)}")
        tb = word_tables(tokens)
        self.vocab = dict(tokens=tokens, size=len(tokens), sep_id=tokens.index(END_TOKENS[0]), pad_id=tokens.index(END_TOKENS[1]),
                          empty_key=tb["empty_key"], **{k: tb[k].to(self.device) for k in ("tok_key", "tail_key", "tail_pow")})
        return self

    def set_references(self, texts=None):
        """The reference words of every item, as padded key rows ref_key int64 [n, W] and counts ref_n int32 [n] on the device.
        texts: the raw reports (the reference's gt_caption), keyed on the host as text.split(' '); None: the bank's own report rows,
        through one mv_bleu_words launch (data sets that keep only ids; needs set_vocab).  Refused: a report of more than 1024 words,
        a count of texts other than the bank's."""
        from . import hip_ops as ops
        from .report_eval import text_keys
        if self.n_texts == 0:
            raise ValueError("set_references: the bank holds no reports (add_reports)")
        if texts is None:
            if self.vocab is None:
                raise ValueError("set_references(None) words the bank's own rows: set_vocab first")
            v = self.vocab
            self.ref_key, self.ref_n = ops.bleu_words(self.txt_ids, v["tok_key"], v["tail_key"], v["tail_pow"], v["sep_id"], v["pad_id"],
                                                      v["empty_key"])
            return self
        texts = list(texts)
        if len(texts) != self.n_texts:
            raise ValueError(f"set_references: {len(texts)} texts for a bank of {self.n_texts} reports")
        keys, counts = text_keys(texts)
        if keys.shape[1] > ops.BLEU_MAX_WORDS:
            raise ValueError(f"set_references: a report of {keys.shape[1]} words (at most {ops.BLEU_MAX_WORDS})")
        self.ref_key, self.ref_n = keys.to(self.device).contiguous(), counts.to(self.device)
        return self

    def check_eval(self, vocab_size: int):
        """What report_eval.evaluate needs of the bank: images, a vocabulary of the model's size, a reference per item."""
        n = self.n_texts
        if n == 0 or n != self.n_images:
            raise ValueError(f"the bank holds {n} reports and {self.n_images} images: item i is image i with report i")
        if self.vocab is None or self.ref_key is None:
            raise ValueError("the bank has no vocabulary or no references (ReportBank.set_vocab, set_references)")
        if self.vocab["size"] != int(vocab_size):
            raise ValueError(f"the bank's vocabulary has {self.vocab['size']} tokens, the model's {int(vocab_size)}")
        if int(self.ref_key.shape[0]) != n:
            raise ValueError(f"{int(self.ref_key.shape[0])} references for {n} items: call set_references after the last add_reports")

    def add_reports(self, ids, lengths):
        done = self.n_texts
        self.add_texts(ids, lengths)
        n_pred = torch.tensor([min(self.max_pred, max(1, int(round((ln - 1) * self.mask_prob)))) for ln in self._len_host[done:].tolist()],
                              dtype=torch.int32).to(self.device)
        self.n_pred = n_pred if self.n_pred is None else torch.cat([self.n_pred, n_pred])
        return self

    def assemble(self, idx, mode="s2s", key=0, step=0, draws=None):
        from . import hip_ops as ops
        n = self.n_texts
        if n == 0 or self.n_images == 0:
            raise ValueError("ReportBank.assemble: the bank is empty (add_reports, add_images)")
        if n != self.n_images or self.n_pred is None or int(self.n_pred.numel()) != n:
            raise ValueError(f"ReportBank.assemble: {n} reports (add_reports) and {self.n_images} images: item i is image i with report i")
        dev_idx, host_idx = self._indices(idx, n, "items")
        fam_host = self._families(mode, int(dev_idx.numel()))
        host = None if host_idx is None else self.host_descriptors(host_idx, fam_host)
        out = ops.report_assemble(self.txt_ids, self.txt_len, self.n_pred, self.img_feats, self.img_pos, dev_idx, self.max_pred,
                                  family=fam_host.to(self.device), key=key, step=step, draws=draws)
        return self._batch(out, host) + ({k: out[k] for k in ("masked_lm_labels", "masked_pos", "masked_weights")},)


# ---------------------------------------------------------------------------------------------------- VQA bank
VQA_GROUPS = 8                     # mv_vqa_score's group slots
_ANS_TYPE = {"CLOSED": 0, "CLOSED ": 0, "OPEN": 1, "OPEN ": 1}          # data_loader.py:434-437


def vqa_answer_type(t) -> int:
    """0 (closed) / 1 (open) from an integer or the reference's strings (data_loader.py:434-437, with their trailing-space variants);
    anything else is 2, which neither split counts."""
    if isinstance(t, str):
        return _ANS_TYPE.get(t, 2)
    if torch.is_tensor(t):
        t = t.item()
    try:
        v = int(t)
    except (TypeError, ValueError):
        return 2
    return v if v in (0, 1) and v == t else 2


class VqaBank(DeviceBank):
    """A VQA data set resident on the device: question i = (image q_img[i], question i, its sparse soft answers, its answer type, its
    group).  Many questions share one image (VQA-RAD: 315 images for 3,064 training questions, data_loader.py:236-273), so an image
    passes the region encoder once, not once per question, and a batch comes out of one mv_vqa_assemble launch.
      add_images(input_img)   as DeviceBank.add_images, once per distinct image
      add_questions(ids, lengths, image_item, labels, scores, ans_type, group=None)
                              ids int64 [n, T] / lengths [n]: add_texts' layout (tokens + [SEP] + [PAD]..., lengths count the [SEP]);
                              image_item int [n]: the item of the image bank; labels[i] / scores[i]: the answer['labels'] /
                              answer['scores'] sequences of the reference's target files -- ragged, possibly empty or None (an all-zero
                              target, :269-271), a label listed twice keeps its later score like target.scatter_ on the CPU;
                              ans_type[i]: 0 / 1 or the reference's strings (vqa_answer_type); group[i] in [0, 8): the reference's
                              --vqa_rad organ subsets (:180-187), None = group 0.  Refused (ValueError, nothing is added): a label
                              outside [0, n_answers), labels and scores of different length, a score that is not finite, a group
                              outside [0, 8), a negative image item.
      assemble(idx, mode)     -> (cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, ans_labels, ans_type): the arguments of
                              CXRBertForVQA.forward with attn_mask a MaskDesc.  mode "s2s" / "bi" / "bar" or one per sample
                              (ReportBank.assemble's rule; the reference's per-sample draw, :282, stays with the caller).  idx given on
                              the host is checked there (IndexError outside the bank, ValueError when a listed question names an image
                              the image bank does not hold) and the descriptors' host copy comes from the host lengths (no read-back);
                              idx on the device (int32) is clamped into the bank by the kernel.
      dense_targets(idx)      f32 [len(idx), n_answers] built on the host with scatter_: the restated reference (:269-271).
    Storage on the device: q_img int32 [n], ans_ptr int32 [n+1], ans_label int32 [nnz], ans_score f32 [nnz], ans_type int32 [n], group
    int32 [n]; host copies of the lengths, q_img and the answers."""

    def __init__(self, model=None, device=None, feat_dtype=None, n_answers=458):
        super().__init__(model, device, feat_dtype)
        self.n_answers = int(n_answers)
        if self.n_answers < 1:
            raise ValueError("VqaBank: n_answers >= 1")
        self.q_img = self.ans_label = self.ans_score = self.ans_type = self.group = None
        self.ans_ptr = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._q_img_host = torch.zeros(0, dtype=torch.int64)
        self._ptr_host = torch.zeros(1, dtype=torch.int64)
        self._label_host = torch.zeros(0, dtype=torch.int64)
        self._score_host = torch.zeros(0, dtype=torch.float32)

    @property
    def n_questions(self):
        return 0 if self.q_img is None else int(self.q_img.numel())

    def add_questions(self, ids, lengths, image_item, labels, scores, ans_type, group=None):
        ids = torch.as_tensor(ids)
        n = int(ids.shape[0]) if ids.dim() == 2 else -1
        img = torch.as_tensor(image_item).reshape(-1)
        if n < 1 or img.numel() != n or len(labels) != n or len(scores) != n or len(ans_type) != n or (group is not None and len(group) != n):
            raise ValueError("add_questions: ids [n, T] and one image item, label list, score list, answer type (and group) per question")
        if img.dtype.is_floating_point or img.dtype == torch.bool or int(img.min()) < 0:
            raise ValueError("add_questions: image_item holds non-negative integers")
        lab, sc, ptr = [], [], [int(self._ptr_host[-1])]
        for i in range(n):
            li = [] if labels[i] is None else torch.as_tensor(labels[i]).reshape(-1).tolist()
            si = [] if scores[i] is None else torch.as_tensor(scores[i], dtype=torch.float32).reshape(-1).tolist()
            if len(li) != len(si):
                raise ValueError(f"add_questions: question {i} lists {len(li)} labels and {len(si)} scores")
            if any(int(l) != l or not 0 <= int(l) < self.n_answers for l in li):
                raise ValueError(f"add_questions: question {i} lists a label outside [0, {self.n_answers})")
            lab += [int(l) for l in li]
            sc += si
            ptr.append(ptr[0] + len(lab))
        sc = torch.tensor(sc, dtype=torch.float32)
        if not bool(torch.isfinite(sc).all()):
            raise ValueError("add_questions: a score is not finite")
        if ptr[-1] > 2 ** 31 - 1:
            raise ValueError("add_questions: more than 2^31 - 1 answers")
        grp = torch.zeros(n, dtype=torch.int64) if group is None else torch.as_tensor(group).reshape(-1).to(torch.int64)
        if int(grp.min()) < 0 or int(grp.max()) >= VQA_GROUPS:
            raise ValueError(f"add_questions: a group outside [0, {VQA_GROUPS})")
        typ = torch.tensor([vqa_answer_type(t) for t in ans_type], dtype=torch.int32)
        self.add_texts(ids, lengths)                         # (its own refusals come before anything of the questions is stored)
        lab = torch.tensor(lab, dtype=torch.int64)
        self._q_img_host = torch.cat([self._q_img_host, img.to(torch.int64).cpu()])
        self._ptr_host = torch.cat([self._ptr_host, torch.tensor(ptr[1:], dtype=torch.int64)])
        self._label_host, self._score_host = torch.cat([self._label_host, lab]), torch.cat([self._score_host, sc])
        cat = lambda old, new: new if old is None else torch.cat([old, new])
        dev32 = lambda t: t.to(torch.int32).to(self.device).contiguous()
        self.q_img = cat(self.q_img, dev32(img))
        self.ans_label, self.ans_score = cat(self.ans_label, dev32(lab)), cat(self.ans_score, sc.to(self.device))
        self.ans_type, self.group = cat(self.ans_type, typ.to(self.device)), cat(self.group, dev32(grp))
        self.ans_ptr = dev32(self._ptr_host)
        return self

    def dense_targets(self, idx):
        idx = torch.as_tensor(idx).reshape(-1).to(torch.int64).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_questions):
            raise IndexError(f"idx outside the bank of {self.n_questions} questions")
        out = torch.zeros((idx.numel(), self.n_answers), dtype=torch.float32)
        for i, d in enumerate(idx.tolist()):
            e0, e1 = int(self._ptr_host[d]), int(self._ptr_host[d + 1])
            if e1 > e0:
                out[i].scatter_(0, self._label_host[e0:e1], self._score_host[e0:e1])
        return out

    def _check_filled(self):
        n = self.n_questions
        if n == 0 or self.n_images == 0:
            raise ValueError("VqaBank: the bank is empty (add_questions, add_images)")
        if n != self.n_texts:
            raise ValueError(f"VqaBank: {self.n_texts} text rows for {n} questions: fill the bank with add_questions, not add_texts")

    def host_idx(self, idx):
        """A host index list, checked against both banks: -> int64 [B]."""
        self._check_filled()
        return self._check_images(self._index_list(idx, self.n_questions, "questions"))

    def _check_images(self, host_idx):
        if int(self._q_img_host.index_select(0, host_idx).max()) >= self.n_images:
            raise ValueError(f"a listed question names an image outside the image bank of {self.n_images}")
        return host_idx

    def assemble(self, idx, mode="bi"):
        from . import hip_ops as ops
        self._check_filled()
        dev_idx, host_idx = self._indices(idx, self.n_questions, "questions")
        if host_idx is not None:
            self._check_images(host_idx)
        fam_host = self._families(mode, int(dev_idx.numel()))
        host = None if host_idx is None else self.host_descriptors(host_idx, fam_host)
        out = ops.vqa_assemble(self.txt_ids, self.txt_len, self.q_img, self.ans_ptr, self.ans_label, self.ans_score, self.ans_type,
                               self.img_feats, self.img_pos, dev_idx, self.n_answers, family=fam_host.to(self.device))
        return self._batch(out, host) + (out["target"], out["ans_type"])


# ---------------------------------------------------------------------------------------------------- classification bank
CLF_MAX_CLASSES = 1024             # mv_clf_assemble / mv_clf_counts


class ClassificationBank(DeviceBank):
    """A diagnosis-classification data set resident on the device: sample i = (image s_img[i], text i, its multi-hot target), what the
    reference's JsonlDataset + collate_fn build per sample on the host and push across every step (Downstream_task/Classification/mmbt/
    data/dataset.py:36-85, data/helpers.py:73-98).  An image passes the region encoder once, a batch comes out of one mv_clf_assemble
    launch, and a whole evaluation's metrics follow from one mv_clf_counts launch over the stored label bits.
      add_images(input_img)   as DeviceBank.add_images, once per distinct image
      add_samples(ids, lengths, labels, image_item=None)
                              ids int64 [n, T] / lengths [n]: add_texts' layout (tokens + [SEP] + [PAD]..., lengths count the [SEP]) --
                              what dataset.py:39-44,80-81 leaves after it drops the leading [SEP]; labels: a multi-hot [n, C] array (any
                              value > 0.5 is set) or one ragged list of class indices per sample (None or empty: an all-zero target; a
                              repeated index is allowed); image_item int [n]: the item of the image bank, None = item i is image i counted
                              from the samples already in the bank.  Mapping label strings to indices (the reference's '' -> 'Others'
                              included, :58-64) and drop_img_percent (one grey image, image_item pointing at it) stay with the caller.
                              Refused (ValueError, nothing is added): an index outside [0, C), a multi-hot array of another width, a
                              negative or non-integer image_item, wrong counts.
      assemble(idx, mode)     -> (cls_tok, input_txt, attn_mask, segment, input_img, sep_tok, target): the arguments of
                              CXRBertForClassification.forward with attn_mask a MaskDesc and target f32 [B, C].  mode "s2s" / "bi" / "bar"
                              or one per sample (ReportBank.assemble's rule); the default "bi" is the 1-D family, the reference's
                              mask_tensor.  idx given on the host is checked there (IndexError outside the bank, ValueError when a listed
                              sample names an image the image bank does not hold) and the descriptors' host copy comes from the host
                              lengths (no read-back); idx on the device (int32) is clamped into the bank by the kernel.
      dense_targets(idx)      f32 [len(idx), C] built on the host: the restated reference (:57-64).
      pos_weight()            f32 [C] as get_criterion forms it (mmbt/main.py:96-98) over the bank's samples.
    Storage on the device: s_img int32 [n], lab_bits int32 [n, W], W = ceil(C / 32), class c = bit c % 32 of word c / 32; host copies of
    the lengths, s_img and the bits."""

    def __init__(self, model=None, device=None, feat_dtype=None, n_classes=14):
        super().__init__(model, device, feat_dtype)
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= CLF_MAX_CLASSES:
            raise ValueError(f"ClassificationBank: 1 <= n_classes <= {CLF_MAX_CLASSES}")
        self.n_words = (self.n_classes + 31) // 32
        self.s_img = self.lab_bits = None
        self._s_img_host = torch.zeros(0, dtype=torch.int64)
        self._bits_host = torch.zeros((0, self.n_words), dtype=torch.int32)

    @property
    def n_samples(self):
        return 0 if self.s_img is None else int(self.s_img.numel())

    def _multi_hot(self, labels, n):
        """labels -> bool [n, C] on the host."""
        C = self.n_classes
        dense = None
        if torch.is_tensor(labels) and labels.dim() == 2:
            dense = labels.detach().cpu()
        elif hasattr(labels, "ndim") and getattr(labels, "ndim") == 2 and getattr(labels, "dtype", None) != object:
            dense = torch.as_tensor(labels)
        if dense is not None:
            if tuple(dense.shape) != (n, C):
                raise ValueError(f"add_samples: a multi-hot label array is [n, C] = [{n}, {C}], got {tuple(dense.shape)}")
            return dense.to(torch.float64) > 0.5
        if len(labels) != n:
            raise ValueError("add_samples: one label list per sample")
        hot = torch.zeros((n, C), dtype=torch.bool)
        for i in range(n):
            li = [] if labels[i] is None else torch.as_tensor(labels[i]).reshape(-1).tolist()
            if any(int(l) != l or not 0 <= int(l) < C for l in li):
                raise ValueError(f"add_samples: sample {i} lists a class outside [0, {C})")
            if li:
                hot[i, [int(l) for l in li]] = True
        return hot

    def _pack(self, hot):
        """bool [n, C] -> int32 [n, W]: class c is bit c % 32 of word c / 32."""
        n, C, W = int(hot.shape[0]), self.n_classes, self.n_words
        padded = torch.zeros((n, W * 32), dtype=torch.int64)
        padded[:, :C] = hot.to(torch.int64)
        words = (padded.view(n, W, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=2)          # in [0, 2^32)
        return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)

    def _unpack(self, bits):
        """int32 [m, W] -> bool [m, C]."""
        w = bits.to(torch.int64) & 0xFFFFFFFF
        return ((w.unsqueeze(2) >> torch.arange(32, dtype=torch.int64)) & 1).reshape(bits.shape[0], -1)[:, :self.n_classes].bool()

    def add_samples(self, ids, lengths, labels, image_item=None):
        ids = torch.as_tensor(ids)
        n = int(ids.shape[0]) if ids.dim() == 2 else -1
        if n < 1 or labels is None:
            raise ValueError("add_samples: ids [n, T], one length and one label row or list (and image item) per sample")
        if image_item is None:
            img = torch.arange(self.n_samples, self.n_samples + n, dtype=torch.int64)
        else:
            img = torch.as_tensor(image_item).reshape(-1)
            if img.numel() != n:
                raise ValueError("add_samples: one image item per sample")
            if img.dtype.is_floating_point or img.dtype == torch.bool or int(img.min()) < 0 or int(img.max()) > 2 ** 31 - 1:
                raise ValueError("add_samples: image_item holds non-negative integers")
            img = img.to(torch.int64).cpu()
        bits = self._pack(self._multi_hot(labels, n))
        self.add_texts(ids, lengths)                         # (its own refusals come before anything of the samples is stored)
        self._s_img_host = torch.cat([self._s_img_host, img])
        self._bits_host = torch.cat([self._bits_host, bits])
        cat = lambda old, new: new if old is None else torch.cat([old, new])
        self.s_img = cat(self.s_img, img.to(torch.int32).to(self.device).contiguous())
        self.lab_bits = cat(self.lab_bits, bits.to(self.device).contiguous())
        return self

    def dense_targets(self, idx):
        idx = torch.as_tensor(idx).reshape(-1).to(torch.int64).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_samples):
            raise IndexError(f"idx outside the bank of {self.n_samples} samples")
        return self._unpack(self._bits_host.index_select(0, idx)).to(torch.float32)

    def pos_weight(self):
        n = self.n_samples
        if n == 0:
            raise ValueError("ClassificationBank.pos_weight: the bank is empty (add_samples)")
        freqs = self._unpack(self._bits_host).sum(dim=0).tolist()
        if min(freqs) == 0:
            raise ValueError(f"ClassificationBank.pos_weight: class {freqs.index(0)} has no positive sample (the reference would hand "
                             "BCEWithLogitsLoss an infinite weight)")
        negative = [n - f for f in freqs]
        return (torch.FloatTensor(freqs) / torch.FloatTensor(negative)) ** -1          # main.py:96-98, verbatim

    def _check_filled(self):
        n = self.n_samples
        if n == 0 or self.n_images == 0:
            raise ValueError("ClassificationBank: the bank is empty (add_samples, add_images)")
        if n != self.n_texts:
            raise ValueError(f"ClassificationBank: {self.n_texts} text rows for {n} samples: fill the bank with add_samples, not add_texts")

    def host_idx(self, idx):
        """A host index list, checked against both banks: -> int64 [B]."""
        self._check_filled()
        return self._check_images(self._index_list(idx, self.n_samples, "samples"))

    def _check_images(self, host_idx):
        if int(self._s_img_host.index_select(0, host_idx).max()) >= self.n_images:
            raise ValueError(f"a listed sample names an image outside the image bank of {self.n_images}")
        return host_idx

    def assemble(self, idx, mode="bi"):
        from . import hip_ops as ops
        self._check_filled()
        dev_idx, host_idx = self._indices(idx, self.n_samples, "samples")
        if host_idx is not None:
            self._check_images(host_idx)
        fam_host = self._families(mode, int(dev_idx.numel()))
        host = None if host_idx is None else self.host_descriptors(host_idx, fam_host)
        out = ops.clf_assemble(self.txt_ids, self.txt_len, self.s_img, self.lab_bits, self.img_feats, self.img_pos, dev_idx,
                               self.n_classes, family=fam_host.to(self.device))
        return self._batch(out, host) + (out["target"],)
