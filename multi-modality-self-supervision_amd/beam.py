"""Beam-search bookkeeping of report generation, kept apart from the model so that it runs (and is tested) on the CPU.

Follows the reference's BertForSeq2SeqDecoder.beam_search
(Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:1239-1467) step for step:
  step 0       top-K of the single beam's log-probs; back pointers 0
  step t > 0   candidate score = log-prob + running score, -10000 more when the beam's last word was EOS; top-K of the K*K
               candidates per sample; back pointer = candidate // K
  final pick   per sample, over the frames up to the first frame whose K words are all EOS: a candidate counts when its word is EOS or
               it lies in that last frame; maximise score + length_penalty * (frame + 1), then follow the back pointers.
The min_len rule (EOS log-prob := -10000 for the first min_len steps) is applied where the log-probs are made (mv_logprob_topk).
n-gram blocking (the reference's forbid_duplicate_ngrams / ngram_size / forbid_ignore_set) is applied there too: the histories and
the ban lists live on the device (mv_ngram_ban after every step, mv_logprob_topk_banned at the next; generate()'s
no_repeat_ngram_size / no_repeat_ignore_ids); this class only hands over its parents and word ids.

The KV cache is shared, not copied: every beam owns one row of an int32 slot table (the cache rows it attends to), and re-ordering
the beams re-orders those rows (`reorder_slot_table`).
"""
from __future__ import annotations

import math

import torch


class BeamSearch:
    def __init__(self, batch_size: int, beam_size: int, eos_id: int, length_penalty: float = 0.0):
        self.B, self.K, self.eos_id, self.length_penalty = int(batch_size), int(beam_size), int(eos_id), float(length_penalty)
        self.scores, self.ids, self.ptrs, self.eos_masks = [], [], [], []

    def step(self, kk_scores: torch.Tensor, kk_ids: torch.Tensor):
        """kk_scores / kk_ids [B*K, K]: the top-K log-probs and word ids of every beam's MASK row.  At step 0 only each sample's first
        beam is read (the reference expands from one beam).  Returns (back_ptrs [B,K] int64 in 0..K-1, word ids [B,K] int64)."""
        B, K = self.B, self.K
        kk_scores = kk_scores.float().view(B, K, K)
        kk_ids = kk_ids.long().view(B, K, K)
        if not self.scores:
            k_scores, k_ids = kk_scores[:, 0, :].clone(), kk_ids[:, 0, :].clone()
            back = torch.zeros((B, K), dtype=torch.int64, device=k_ids.device)
        else:
            cand = kk_scores + (self.eos_masks[-1] * -10000.0 + self.scores[-1]).unsqueeze(-1)
            k_scores, pick = torch.topk(cand.reshape(B, K * K), k=K)
            back = torch.div(pick, K, rounding_mode="floor")
            k_ids = torch.gather(kk_ids.reshape(B, K * K), 1, pick)
        self.ptrs.append(back)
        self.ids.append(k_ids)
        self.eos_masks.append((k_ids == self.eos_id).float())
        self.scores.append(k_scores)
        return back, k_ids

    def parents(self, back: torch.Tensor) -> torch.Tensor:
        """Flat parent beam (b*K + back) of every new beam, int64 [B*K]."""
        base = torch.arange(self.B, device=back.device).unsqueeze(1) * self.K
        return (base + back).reshape(-1)

    def all_done(self) -> torch.Tensor:
        """Device bool: every sample has had a frame whose K words are all EOS (nothing after it changes the result)."""
        fin = torch.zeros(self.B, dtype=torch.bool, device=self.ids[0].device)
        for m in self.eos_masks:
            fin |= m.bool().all(dim=1)
        return fin.all()

    def finalize(self, max_len: int, pad_id: int = 0):
        """-> (ids int64 [B, max_len] padded with pad_id, scores f32 [B] (score + length penalty of the pick; -inf when none),
        traces {'pred_seq', 'scores', 'wids', 'ptrs'} padded to max_len along the step axis as the reference returns them)."""
        scores = torch.stack(self.scores, 1).cpu().tolist()           # [B][frames][K]
        wids = torch.stack(self.ids, 1).cpu().tolist()
        ptrs = torch.stack(self.ptrs, 1).cpu().tolist()
        out = torch.full((self.B, max_len), pad_id, dtype=torch.int64)
        best = torch.full((self.B,), -math.inf, dtype=torch.float32)
        seqs = []
        for b in range(self.B):
            sc, wl, pt = scores[b], wids[b], ptrs[b]
            last = len(sc) - 1
            for i, w in enumerate(wl):
                if all(x == self.eos_id for x in w):
                    last = i
                    break
            mx, fid, pos = -math.inf, -1, -1
            for f in range(last + 1):
                for i, w in enumerate(wl[f]):
                    if w == self.eos_id or f == last:
                        s = sc[f][i] + self.length_penalty * (f + 1)
                        if s > mx:
                            mx, fid, pos = s, f, i
            if fid == -1:
                seq = [0]
            else:
                seq = [wl[fid][pos]]
                for f in range(fid, 0, -1):
                    pos = pt[f][pos]
                    seq.append(wl[f - 1][pos])
                seq.reverse()
            seqs.append(seq)
            out[b, :len(seq)] = torch.tensor(seq[:max_len], dtype=torch.int64)
            best[b] = mx
        F = len(scores[0])
        traces = {"pred_seq": out.clone(),
                  "scores": torch.zeros((self.B, max_len, self.K), dtype=torch.float32),
                  "wids": torch.zeros((self.B, max_len, self.K), dtype=torch.int64),
                  "ptrs": torch.zeros((self.B, max_len, self.K), dtype=torch.int64)}
        traces["scores"][:, :F] = torch.tensor(scores, dtype=torch.float32)
        traces["wids"][:, :F] = torch.tensor(wids, dtype=torch.int64)
        traces["ptrs"][:, :F] = torch.tensor(ptrs, dtype=torch.int64)
        return out, best, traces


def reorder_slot_table(table: torch.Tensor, parents: torch.Tensor, col0: int, col1: int) -> torch.Tensor:
    """In place: the history columns [col0, col1) of every beam's slot-table row become those of its parent beam (the KV cache itself
    is not touched).  table int32 [B*K, cols]; parents int64 [B*K] (BeamSearch.parents)."""
    if col1 > col0:
        table[:, col0:col1] = table.index_select(0, parents)[:, col0:col1]
    return table
