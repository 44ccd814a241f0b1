"""Shared helpers of the report fine-tuning tests: an fp64 torch restatement of the objective of the reference's
BertForPreTrainingLossMask(tasks='report_generation') and the case table of the kernel tests.  No GPU, no package import.

The restatement, in this project's words (paths relative to Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/):
  * per-slot loss with smoothing: loss.py:28-32 builds a target row that holds label_smoothing / (V - 2) everywhere and 0 in column 0
    (torch.full rounds the smoothing value to f32 when the module is built, loss.py:29); the label's column takes the confidence
    1 - label_smoothing (loss.py:32,45); a row whose label is 0 is zeroed (loss.py:46); the loss is
    sum_c q (log q - log_softmax(z)) with 0 log 0 = 0 (loss.py:48, F.kl_div summed over the vocabulary);
  * without smoothing: CrossEntropyLoss(reduction='none'), no ignore index -- label 0 counts (model.py:929,1050);
  * loss_mask_and_normalize (model.py:998-1005): loss * weights, per-sample sums, the int(B * (1 - drop_worst_ratio)) smallest sums
    are kept, normalised by the kept samples' weight sum + 1e-5.
"""
import numpy as np
import torch


def keep_count(B, ratio):
    return int(B * (1 - ratio))                                  # model.py:1002, the reference's own expression


def smoothing_constants(label_smoothing, V):
    """(confidence, smoothing value): the latter rounded to f32 as the reference's torch.full does."""
    return 1.0 - label_smoothing, float(np.float32(label_smoothing / (V - 2)))


def slot_loss(z, labels, label_smoothing):
    """z [..., V], labels int64 [...] -> f64 [...]: the loss of every listed slot (differentiable in z)."""
    z = z.double()
    V = z.shape[-1]
    logp = torch.log_softmax(z, dim=-1)
    if not label_smoothing:
        return -logp.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
    conf, sval = smoothing_constants(label_smoothing, V)
    q = torch.full_like(logp, sval)
    q[..., 0] = 0.0
    q.scatter_(-1, labels.unsqueeze(-1), conf)
    q = q * (labels != 0).unsqueeze(-1).to(q.dtype)
    return (torch.xlogy(q, q) - q * logp).sum(-1)


def normalise(slot_losses, weights, ratio):
    """loss_mask_and_normalize: slot losses / weights [B, P] -> (loss scalar f64, keep bool [B]).  The k smallest sample sums are kept;
    equal sums go to the lower sample index (a stable ascending sort)."""
    w = weights.double()
    per = (slot_losses.double() * w).sum(-1)
    B = per.shape[0]
    k = keep_count(B, ratio)
    order = torch.sort(per.detach(), stable=True).indices[:k]
    keep = torch.zeros(B, dtype=torch.bool)
    keep[order] = True
    den = w.sum(-1)[keep].sum() + 1e-5
    return (per[keep] / den).sum(), keep


def objective(z, labels, weights, label_smoothing, ratio):
    """The listed form: z [B, P, V], labels / weights [B, P] -> (loss f64, keep bool [B], slot losses f64 [B, P])."""
    sl = slot_loss(z, labels, label_smoothing)
    loss, keep = normalise(sl, weights, ratio)
    return loss, keep, sl


# ------------------------------------------------------------------------------------------------ kernel cases
# Sample templates: (position, label, weight) entries; label -1 stands for V - 1.  Sample b of a case uses template b % 5.
#   0: one row with two entries of equal labels          1: one row with three different labels, fractional weights, label V - 1
#   2: no entries                                         3: label 0 only (ignored under smoothing, counted without)
#   4: a saturated row (+-80) with a second, zero-weight entry, and an all-equal row
TEMPLATES = {
    0: [(3, 10, 1.0), (3, 10, 1.0)],
    1: [(2, 5, 1.0), (2, -1, 0.25), (2, 7, 0.5)],
    2: [],
    3: [(1, 0, 1.0)],
    4: [(6, 3, 1.0), (6, 8, 0.0), (9, 4, 0.75)],
}
# the small vocabulary adds a row whose only entry has weight zero and a second label-0 row
EXTRA = {0: [(7, 11, 0.0)], 3: [(2, 0, 1.0)]}
L_CASE = 16                                                      # positions per sample (flat row = b * L_CASE + position)


def make_case(B, V, ld, seed, extra=True, identical=False):
    """-> dict: the CSR inputs of the kernels (numpy / torch host tensors), the logits [U, ld] f32 (pad columns hold garbage that must
    not be read) and the listed form [B, P] the restatement takes.  `identical`: every sample uses template 1 and the same logits."""
    g = torch.Generator().manual_seed(seed)
    entries = []                                                 # (sample, position, label, weight) in listing order
    for b in range(B):
        t = 1 if identical else b % 5
        for (p, lab, w) in TEMPLATES[t] + (EXTRA.get(t, []) if extra and not identical else []):
            entries.append((b, p, V - 1 if lab < 0 else lab, w))
    flat = sorted({b * L_CASE + p for (b, p, _, _) in entries})
    row_of = {f: u for u, f in enumerate(flat)}
    U = len(flat)
    logits = torch.randn(max(U, 1), ld, generator=g) * 3.0
    logits[:, V:] = 1e30                                         # pad columns: reading one would show at once
    for u, f in enumerate(flat):
        b, p = divmod(f, L_CASE)
        if identical:
            logits[u] = logits[0]
        elif b % 5 == 4 and p == 6:
            logits[u, :40] = 80.0
            logits[u, 40:V] = -80.0
        elif b % 5 == 4 and p == 9:
            logits[u, :V] = 1.5
    logits = logits[:U].contiguous()
    by_row = sorted(range(len(entries)), key=lambda i: (row_of[entries[i][0] * L_CASE + entries[i][1]], i))
    row_ptr = np.zeros(U + 1, np.int32)
    for i in by_row:
        row_ptr[row_of[entries[i][0] * L_CASE + entries[i][1]] + 1] += 1
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    P = max(1, max((sum(1 for e in entries if e[0] == b) for b in range(B)), default=1))
    slot_row = torch.zeros((B, P), dtype=torch.int64)            # padded slots point at row 0 with weight 0
    lab = torch.zeros((B, P), dtype=torch.int64)
    wt = torch.zeros((B, P), dtype=torch.float64)
    fill = [0] * B
    slot_of_entry = []
    for (b, p, l_, w) in entries:
        j = fill[b]
        fill[b] += 1
        slot_row[b, j], lab[b, j], wt[b, j] = row_of[b * L_CASE + p], l_, w
        slot_of_entry.append((b, j))
    return dict(B=B, V=V, ld=ld, U=U, n=len(entries), logits=logits, row_ptr=torch.from_numpy(row_ptr),
                labels=torch.tensor([entries[i][2] for i in by_row], dtype=torch.int32),
                weights=torch.tensor([entries[i][3] for i in by_row], dtype=torch.float32),
                sample=torch.tensor([entries[i][0] for i in by_row], dtype=torch.int32),
                entry_slot=[slot_of_entry[i] for i in by_row], slot_row=slot_row, slot_labels=lab, slot_weights=wt)


def reference(case, label_smoothing, ratio, scale=1.0):
    """fp64 restatement over a case -> dict(loss, keep [B] bool, entry_loss [n] in CSR order, grad [U, V] = scale * d loss / d logits)."""
    V, U = case["V"], case["U"]
    z = case["logits"][:, :V].double().clone().requires_grad_(True)
    listed = z[case["slot_row"].reshape(-1)].reshape(*case["slot_row"].shape, V) if U else torch.zeros(*case["slot_row"].shape, V, dtype=torch.float64)
    loss, keep, sl = objective(listed, case["slot_labels"], case["slot_weights"], label_smoothing, ratio)
    grad = torch.zeros(U, V, dtype=torch.float64)
    if U and loss.requires_grad:
        grad = torch.autograd.grad(loss, z, allow_unused=True)[0]
        grad = torch.zeros(U, V, dtype=torch.float64) if grad is None else grad
    entry_loss = torch.tensor([float(sl[b, j].detach()) for (b, j) in case["entry_slot"]], dtype=torch.float64)
    return dict(loss=float(loss), keep=keep, entry_loss=entry_loss, grad=grad * scale)
