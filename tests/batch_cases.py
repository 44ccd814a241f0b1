"""Cases, restated kernels, references and the judgement of the batch-assembly and row-plan kernels (csrc/mv_batch.hip: mv_mlm_draws,
mv_mlm_corrupt with its label-index pass, mv_pack_plan, mv_tail_perm) and of their composition as the engine runs it (`chain`).

Plain module: nothing here touches the GPU or the HIP library.  tests/test_batch_sweep_gpu.py runs the cases on the device,
tests/test_batch_cases_cpu.py counts the branches they reach, reads the constants out of the sources and plants defects.

* every case is a cfg dict; `*_inputs(cfg)` derives every tensor from cfg["seed"] (and the other cfg fields) alone;
* `*_reference` is the operation the plain way (Python loops, np.nonzero, np.cumsum, a stable sort; oracle.data_oracle.random_word and
  assemble_sample for the corruption): for every output buffer it gives the expected value of every element AND a boolean mask of the
  elements the contract writes;
* `*_restated` is the kernel's own algorithm in numpy -- blocks of 256 threads, waves of 64, strided trips, per-wave counts -- storing
  into sentinel-filled buffers with guard elements through `_store`, which records a store outside the buffer instead of making it.
  `defect` plants one defect at a time;
* `*_judge` is the one judgement both test files apply.  Everything is an integer or an exactly representable f32, so every comparison
  is equality; there is no tolerance anywhere in this module.

What the cases cannot tell apart, and therefore do not claim to test: evaluating u / 0.15 in f32 instead of double.  A check on the
CPU found no difference in outcome at any point of the 2^-24 grid below 0.15, nor at any f32 within 8 ulps of 0.15, 0.12 or 0.135.
For the same reason the two `<=` defects are planted in the only form in which they can change an outcome: no f32 u equals the double
0.15 and no f32 u has u / 0.15 == 0.8 in double, so `<=` evaluated in double is the same function as `<`; compared against the f32
constants (`u <= 0.15f`, `u / 0.15f <= 0.8f`) it selects u = f32(0.15) and masks u = nextafter(f32(0.12), 1).
"""
import numpy as np

import rowops_cases as R

# ---- constants of csrc/mv_batch.hip and csrc/mv_common.h (tests/test_batch_cases_cpu.py reads the same numbers out of the sources) ----
NT = 256                      # threads per block of the four one-block-per-sample kernels, and of mlm_draws_kernel
WAVE = 64
TP_MAXL = 2048                # rows of one sample mv_tail_perm holds flags for
TOK_PAD, TOK_SEP, TOK_MASK = 0, 102, 103
P_SELECT, P_MASK, P_RANDOM = 0.15, 0.8, 0.9
IGNORE = -100
HASH_MUL, HASH_SHIFT = R.HASH_MUL, R.HASH_SHIFT
VOCAB = 30522

GUARD = 16                    # elements in front of and behind every output buffer
SENTINEL = -7777777           # integer buffers: neither -1 (no such row) nor -100 (no label) nor any id or row
I32, I64, F32 = np.int32, np.int64, np.float32

FAMILY_ID = {"full": 0, "s2s": 1, "bar": 2, "noncross": 3, "1d": 4}


def case_id(cfg):
    def s(v):
        return "x".join(str(i) for i in v) if isinstance(v, (tuple, list)) else (hex(v) if isinstance(v, int) and v > 1 << 31 else str(v))
    return "%s%d-" % (cfg["fam"], cfg["seed"]) + "-".join("%s%s" % (k, s(v)) for k, v in cfg.items() if k not in ("fam", "seed"))


# =====================================================================================================================
# buffers and the judgement
# =====================================================================================================================
def new_buffers(specs):
    """specs: name -> (dtype, n).  -> name -> flat array of n + 2 * GUARD elements holding the sentinel (NaN for f32)"""
    return {k: np.full(n + 2 * GUARD, np.nan if dt is F32 else SENTINEL, dtype=dt) for k, (dt, n) in specs.items()}


def _store(bufs, name, idx, val):
    """the only store of the restated kernels: element idx (array) of buffer `name` <- val; a store outside the flat buffer is recorded"""
    flat = bufs[name]
    j = np.asarray(idx, dtype=np.int64).reshape(-1) + GUARD
    val = np.broadcast_to(np.asarray(val), j.shape)
    inside = (j >= 0) & (j < flat.size)
    flat[j[inside]] = val[inside]
    if not inside.all():
        bufs.setdefault("_oob", []).append((name, int(j[~inside][0]) - GUARD))


def _body(bufs, name):
    return bufs[name][GUARD:bufs[name].size - GUARD]


def _held(flat):
    return np.isnan(flat) if flat.dtype == F32 else flat == SENTINEL


def judge_buffers(specs, ref, out):
    """out: name -> flat array, guards included, as new_buffers makes them.  ref: name -> (expected [n], written bool [n]).
    Where `written`, the element equals the expected value; everywhere else -- guards, unwritten tails, buffers passed as NULL --
    the sentinel is still there."""
    what = []
    for name, (dt, n) in specs.items():
        flat = np.asarray(out[name])
        if flat.dtype != dt or flat.shape != (n + 2 * GUARD,):
            what.append("%s: %s %s, expected %s [%d]" % (name, flat.dtype, flat.shape, np.dtype(dt), n + 2 * GUARD))
            continue
        want, written = ref[name]
        want, written = np.asarray(want).reshape(-1), np.asarray(written).reshape(-1)
        assert want.shape == written.shape == (n,) and want.dtype == dt, name
        assert not _held(want[written]).any(), name                             # the sentinel cannot be a result
        held, body = _held(flat), flat[GUARD:GUARD + n]
        if not (held[:GUARD].all() and held[GUARD + n:].all()):
            what.append("%s: a guard element was overwritten" % name)
        bad = written & (body != want)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            what.append("%s[%d] = %r, expected %r (%d wrong)" % (name, i, body[i], want[i], int(bad.sum())))
        extra = ~written & ~held[GUARD:GUARD + n]
        if extra.any():
            i = int(np.nonzero(extra)[0][0])
            what.append("%s[%d] = %r written where the contract writes nothing (%d such)" % (name, i, body[i], int(extra.sum())))
    if out.get("_oob"):
        what.append("store outside the buffer: %s[%d]" % out["_oob"][0])
    return (not what, "; ".join(what))


def _all(values, dt):
    v = np.asarray(values, dtype=dt).reshape(-1)
    return v, np.ones(v.shape, dtype=bool)


def _none(n, dt):
    return np.zeros(n, dtype=dt), np.zeros(n, dtype=bool)


def _head(values, n, dt):
    """the first len(values) of n elements are written"""
    v, w = np.zeros(n, dtype=dt), np.zeros(n, dtype=bool)
    v[:len(values)] = values
    w[:len(values)] = True
    return v, w


# =====================================================================================================================
# mv_mlm_draws
# =====================================================================================================================
def draw_values(counter, key, vocab):
    """u = (h(2i) >> 8) * 2^-24 (f32, exact), rnd = (h(2i+1) * vocab) >> 32 (int32) for an array of token counters i"""
    i = np.asarray(counter, dtype=np.uint64)
    h0, h1 = R.hash32(2 * i, key), R.hash32(2 * i + 1, key)
    u = ((h0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(F32)
    rnd = ((h1 * np.uint64(vocab)) >> np.uint64(32)).astype(I32)
    return u, rnd


def draw_stream(key, B, S, vocab):
    """(u f32 [B, S], rnd int32 [B, S]) with token (b, t) at counter i = b*S + t"""
    i = np.array([[b * S + t for t in range(S)] for b in range(B)], dtype=np.uint64)
    return draw_values(i, key, vocab)


KEY_LO = 0x00000000C0FFEE11       # a zero high word
KEY_HI = 0x5EED1234ABCDEF12
DRAW_VOCABS = (1, 2, VOCAB, 2 ** 31 - 1)


def draws_cases():
    shapes = [(1, 1, "none"), (5, 51, "2B"), (15, 17, "SB"), (16, 16, "2B"), (1, 256, "none"), (1, 257, "SB"), (257, 1, "none"), (1, 773, "none"),
              (3, 85, "SB"), (2, 128, "2B")]
    out = []
    for s, (B, S, pair) in enumerate(shapes):
        out.append(dict(fam="draws", seed=s, B=B, S=S, vocab=DRAW_VOCABS[s % 4], key=(KEY_LO, KEY_HI)[(s // 2) % 2] + s, pair=pair))
    out.append(dict(fam="draws", seed=len(out), B=64, S=12, vocab=VOCAB, key=KEY_HI, pair="none"))
    out.append(dict(fam="draws", seed=len(out), B=7, S=37, vocab=2 ** 31 - 1, key=KEY_LO, pair="SB"))
    return out


def draws_shape2(cfg):
    return {"none": None, "2B": (2 * cfg["B"], cfg["S"]), "SB": (cfg["S"], cfg["B"])}[cfg["pair"]]


def draws_buffers(cfg):
    n = cfg["B"] * cfg["S"]
    specs = dict(u=(F32, n), rnd=(I32, n))
    if draws_shape2(cfg):
        B2, S2 = draws_shape2(cfg)
        specs.update(u2=(F32, B2 * S2), rnd2=(I32, B2 * S2))
    return specs


def draws_inputs(cfg):
    return dict(key=cfg["key"], vocab=cfg["vocab"])


def draws_branch(cfg):
    n = cfg["B"] * cfg["S"]
    b = ["n=%d" % n, "vocab=%d" % cfg["vocab"], "key_hi=0" if cfg["key"] >> 32 == 0 else "key_hi!=0", "pair_" + cfg["pair"]]
    b.append("blocks=1" if n <= NT else "blocks>1")
    b.append("last_block_full" if n % NT == 0 else "last_block_partial")
    if cfg["B"] > 1 and cfg["S"] > 1:
        b.append("B>1_and_S>1")
    return b


def draws_reference(cfg, inp):
    ref = {}
    u, rnd = draw_stream(inp["key"], cfg["B"], cfg["S"], inp["vocab"])
    ref["u"], ref["rnd"] = _all(u, F32), _all(rnd, I32)
    if draws_shape2(cfg):
        u2, rnd2 = draw_stream(inp["key"], *draws_shape2(cfg), inp["vocab"])
        ref["u2"], ref["rnd2"] = _all(u2, F32), _all(rnd2, I32)
    return ref


def _draws_kernel(bufs, names, key, B, S, vocab, defect):
    n = B * S
    for blk in range((n + NT - 1) // NT):
        i = blk * NT + np.arange(NT)
        i = i[i < n]
        c = ((i % S) * B + i // S if defect == "index_transposed" else i).astype(np.uint64)
        h0, h1 = R.hash32(2 * c, key), R.hash32(2 * c + 1, key)
        m = (h0 & np.uint64(0xffffff)) if defect == "u_low24" else (h0 >> np.uint64(8))
        _store(bufs, names[0], i, m.astype(F32) * F32(1.0 / 16777216.0))
        r = (h1 % np.uint64(vocab)) if defect == "rnd_mod" else ((h1 * np.uint64(vocab)) >> np.uint64(32))
        _store(bufs, names[1], i, r.astype(I32))


def draws_restated(cfg, inp, defect=None):
    bufs = new_buffers(draws_buffers(cfg))
    _draws_kernel(bufs, ("u", "rnd"), inp["key"], cfg["B"], cfg["S"], inp["vocab"], defect)
    if draws_shape2(cfg):
        _draws_kernel(bufs, ("u2", "rnd2"), inp["key"], *draws_shape2(cfg), inp["vocab"], defect)
    return bufs


def draws_judge(cfg, inp, ref, out):
    ok, what = judge_buffers(draws_buffers(cfg), ref, out)
    if ok and draws_shape2(cfg):                      # the stream depends on (b, t) through b*S + t alone
        n = cfg["B"] * cfg["S"]
        for a, b in (("u", "u2"), ("rnd", "rnd2")):
            if not np.array_equal(out[a][GUARD:GUARD + n], out[b][GUARD:GUARD + n]):
                ok, what = False, "%s and %s differ on their common prefix" % (a, b)
    return ok, what


# =====================================================================================================================
# mv_mlm_corrupt (mlm_corrupt_kernel + label_index_kernel)
# =====================================================================================================================
class Replay:
    """python `random` stand-in replaying per-token draws: random() -> u[i] for token i, randrange() -> rnd[i]"""

    def __init__(self, u, r):
        self.u, self.r, self.i = u, r, -1

    def random(self):
        self.i += 1
        return float(self.u[self.i])

    def randrange(self, n):
        return int(self.r[self.i])


def edge_draws():
    """the f32 neighbours of 0.15, 0.12 and 0.135 (each, the one below, the one above), 0 and the largest u"""
    e = np.array([0.15, 0.12, 0.135], dtype=F32)
    return np.concatenate([e, np.nextafter(e, F32(0.0)), np.nextafter(e, F32(1.0)), np.array([0.0, 0.99999994], dtype=F32)]).astype(F32)


U_RANDOM = F32(0.125)         # u / 0.15 = 0.8333: the random-id branch
U_MASK = F32(0.1)
U_KEEP = F32(0.14)
RND_PLANTED = (0, TOK_SEP, TOK_MASK)
CORRUPT_L = (8, 255, 256, 257, 513)
CORRUPT_N = (0, 1, 36, 254, 300)
CORRUPT_B = (1, 7, 257, 300)          # 300: block b >= 257 is the first to take a second trip of the loop over counts[0..b)
CORRUPT_DRAWS = ("hash", "edges", "zero", "half", "last_only", "lanes", "wave")


def corrupt_cases():
    rows = [  # B, N, S, lens, draws, family, desc, index
        (1, 0, 5, "edges", "hash"), (7, 1, 4, "edges", "half"), (7, 0, 5, "edges", "hash"), (7, 1, 4, "edges", "zero"),
        (1, 1, 4, "edges", "half"), (1, 0, 5, "edges", "last_only"),
        (7, 36, 216, "edges", "edges"), (7, 36, 217, "edges", "hash"), (7, 0, 253, "full", "zero"), (1, 1, 253, "full", "lanes"),
        (7, 36, 218, "edges", "last_only"), (7, 254, 256, "full", "lanes"), (7, 300, 210, "edges", "half"), (7, 254, 256, "edges", "half"),
        (7, 254, 256, "full", "wave"), (1, 36, 217, "full", "wave"), (7, 300, 210, "random", "edges"), (7, 254, 256, "random", "hash"),
        (257, 0, 5, "edges", "hash"), (257, 1, 4, "edges", "zero"), (300, 1, 4, "edges", "hash"), (300, 0, 5, "full", "zero"),
        (300, 0, 5, "edges", "last_only"),
        (7, 36, 217, "random", "hash", "null", "given", "given"), (7, 36, 217, "random", "hash", "given", "null", "given"),
        (7, 36, 217, "random", "edges", "given", "given", "null"), (7, 1, 4, "edges", "hash", "null", "null", "null"),
        (7, 36, 217, "edges", "zero"), (7, 36, 217, "full", "zero"), (1, 36, 217, "edges", "edges"), (1, 36, 217, "edges", "half"),
        (1, 36, 217, "edges", "zero"), (1, 36, 217, "edges", "hash"), (1, 36, 217, "edges", "lanes"), (1, 36, 217, "edges", "wave"),
        (7, 36, 474, "full", "zero"), (7, 36, 474, "edges", "lanes"), (1, 0, 510, "full", "lanes"), (7, 36, 474, "random", "hash"),   # text over two trips
    ]
    out = []
    for s, r in enumerate(rows):
        B, N, S, lens, draws = r[:5]
        fam, desc, index = r[5:] if len(r) > 5 else ("given", "given", "given")
        out.append(dict(fam="corrupt", seed=s, B=B, N=N, S=S, lens=lens, draws=draws, family=fam, desc=desc, index=index))
    return out


def _lengths(cfg, rs):
    B, S = cfg["B"], cfg["S"]
    if cfg["lens"] == "full":
        return np.full(B, S, dtype=I32)
    if cfg["lens"] == "random":
        return rs.randint(1, S + 1, size=B).astype(I32)
    edges = [0, 1, S - 1, S, S + 5, -3]
    ln = np.array([edges[(b + cfg["seed"]) % 6] for b in range(B)], dtype=I32)
    if B >= 3:
        ln[0] = ln[B // 2] = ln[B - 1] = 0                  # a zero count in front of, inside and at the end of the prefix sum
    return ln


def clamp_lengths(lengths, S):
    return np.array([min(max(int(v), 0), S) for v in lengths], dtype=np.int64)


def _shape_draws(cfg, u, rnd, ln):
    """the draw class of the case, applied to the hash draws in place"""
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    n2, kind = N + 2, cfg["draws"]
    bl = int(np.argmax(ln))                                 # the longest sample takes the planted values
    at = 0
    if kind == "edges":
        e = edge_draws()
        at = min(S, e.size)
        u[bl, :at] = e[:at]
    if kind in ("hash", "edges"):                           # the random-id branch with the ids 0, [SEP] and [MASK]
        for j, v in enumerate(RND_PLANTED):
            if at + j < S:
                u[bl, at + j], rnd[bl, at + j] = U_RANDOM, v
    elif kind == "zero":
        u[:] = 0.0
    elif kind == "half":
        u[:] = 0.5
    elif kind == "last_only":
        u[:] = 0.5
        for b in range(B):
            if ln[b] > 0:
                u[b, ln[b] - 1] = 0.0
    elif kind == "lanes":                                   # labels at i % 64 in {0, 63}: lanes 0 and 63, threads 0 / 255 of the next trip
        u[:] = 0.5
        for t in range(S):
            if (n2 + t) % WAVE in (0, WAVE - 1):
                u[:, t] = U_MASK
    elif kind == "wave":                                    # one whole wave of labels, and one label behind it
        u[:] = 0.5
        t0 = -n2 % WAVE
        u[:, t0:t0 + WAVE] = U_KEEP
        if t0 + WAVE + 5 < S:
            u[:, t0 + WAVE + 5] = U_RANDOM


def corrupt_inputs(cfg):
    rs = np.random.RandomState(7100 + cfg["seed"])
    B, S = cfg["B"], cfg["S"]
    lengths = _lengths(cfg, rs)
    ids = rs.randint(1000, VOCAB, size=(B, S)).astype(I64)
    u, rnd = draw_stream(KEY_HI ^ (cfg["seed"] * 0x10001), B, S, VOCAB)
    _shape_draws(cfg, u, rnd, clamp_lengths(lengths, S))
    family = rs.randint(0, 5, size=B).astype(I32) if cfg["family"] == "given" else None
    return dict(ids=ids, lengths=lengths, u=u, rnd=rnd, family=family, vocab=VOCAB)


def corrupt_buffers(cfg):
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    T, L = S + 1, S + N + 3
    return dict(input_txt=(I64, B * T), segment=(I64, B * T), txt_labels=(I64, B * L), n_ids=(I32, B), desc=(I32, 3 * B), counts=(I32, B),
                label_rows=(I32, B * S), label_ids=(I32, B * S), n_labels=(I32, 1))


def _corrupt_plain(B, N, S, ids, lengths, u, rnd, family, vocab, desc=True, index=True):
    """-> name -> (expected, written), by oracle.data_oracle on replayed draws and the header's rules where the reference has none"""
    from oracle import data_oracle as DO
    assert (DO.PAD, DO.SEP, DO.MASK) == (TOK_PAD, TOK_SEP, TOK_MASK)
    T, L = S + 1, S + N + 3
    txt, seg, lab = np.zeros((B, T), dtype=I64), np.zeros((B, T), dtype=I64), np.zeros((B, L), dtype=I64)
    n_ids, counts, dsc = np.zeros(B, dtype=I32), np.zeros(B, dtype=I32), np.zeros((B, 3), dtype=I32)
    ln = clamp_lengths(lengths, S)
    for b in range(B):
        n = int(ln[b])
        if n == 0:                                          # the header: [SEP] at t = 0, no label, counts = 0, n_ids = 1
            toks, labs = [], []
        else:
            toks, labs = DO.random_word(ids[b, :n].tolist(), Replay(u[b], rnd[b]), vocab)
        txt[b], lab[b], seg[b], n_ids[b] = DO.assemble_sample(toks, labs, N, S)
        counts[b] = int((lab[b] != IGNORE).sum())
        dsc[b] = (int(family[b]) if family is not None else 0, N + 2, N + 2 + n + 1)
    rows = np.nonzero(lab.reshape(-1) != IGNORE)[0]
    ref = dict(input_txt=_all(txt, I64), segment=_all(seg, I64), txt_labels=_all(lab, I64), n_ids=_all(n_ids, I32), counts=_all(counts, I32),
               desc=_all(dsc, I32) if desc else _none(3 * B, I32))
    if index:
        ref.update(label_rows=_head(rows, B * S, I32), label_ids=_head(lab.reshape(-1)[rows], B * S, I32), n_labels=_all([rows.size], I32))
    else:
        ref.update(label_rows=_none(B * S, I32), label_ids=_none(B * S, I32), n_labels=_none(1, I32))
    return ref


def corrupt_reference(cfg, inp):
    return _corrupt_plain(cfg["B"], cfg["N"], cfg["S"], inp["ids"], inp["lengths"], inp["u"], inp["rnd"], inp["family"], inp["vocab"],
                          desc=cfg["desc"] == "given", index=cfg["index"] == "given")


def _mlm_action(u, defect):
    """0 none, 1 [MASK], 2 random id, 3 keep -- in double, like the python the kernel replaces"""
    p = u.astype(np.float64)
    sel = (u <= F32(P_SELECT)) if defect == "le_0.15" else (p < P_SELECT)
    q = p / P_SELECT
    mask = ((u / F32(P_SELECT)).astype(F32) <= F32(P_MASK)) if defect == "le_0.8" else (q < P_MASK)
    return np.where(~sel, 0, np.where(mask, 1, np.where(q < P_RANDOM, 2, 3)))


def _corrupt_kernels(bufs, B, N, S, ids, lengths, u, rnd, family, desc, index, defect):
    T, L, n2 = S + 1, S + N + 3, N + 2
    tid = np.arange(NT)
    for b in range(B):                                      # mlm_corrupt_kernel: one block per sample
        ln = min(max(int(lengths[b]), 0), S)
        mine = np.zeros(NT, dtype=np.int64)
        for i0 in range(0, L, NT):
            i = i0 + tid
            live = i < L
            t = i - (n2 - 1 if defect == "label_offset_N+1" else n2)
            text = live & (t >= 0) & (t < T)
            tc = np.clip(t, 0, S - 1)
            valid = text & (t < ln)
            act = np.where(valid, _mlm_action(u[b, tc], defect), 0)
            tok = np.where(act == 1, TOK_MASK, np.where(act == 2, rnd[b, tc], ids[b, tc]))
            sep = ln + (1 if defect == "sep_late" else 0)
            tok = np.where(valid, tok, np.where(t == sep, TOK_SEP, TOK_PAD))
            mine += act > 0
            _store(bufs, "input_txt", b * T + t[text], tok[text])
            _store(bufs, "segment", b * T + t[text], 1)
            _store(bufs, "txt_labels", b * L + i[live], np.where(act > 0, ids[b, tc], IGNORE)[live])
        total = int(mine.reshape(NT // WAVE, WAVE).sum(axis=1).sum())           # block_sum: lanes, then the four wave totals
        c = total
        if total == 0 and (ln > 0 or defect == "forced_when_len0"):
            _store(bufs, "txt_labels", b * L + n2, TOK_MASK if defect == "forced_labels_corrupted" else ids[b, 0])
            _store(bufs, "input_txt", b * T, TOK_MASK)
            c = 1
        _store(bufs, "counts", b, c)
        _store(bufs, "n_ids", b, ln + 1)
        if desc:
            _store(bufs, "desc", 3 * b + np.arange(3), [int(family[b]) if family is not None else 0, n2, n2 + ln + 1])
    if not index:
        return
    counts, lab = _body(bufs, "counts"), _body(bufs, "txt_labels")
    for b in range(B):                                      # label_index_kernel: one block per sample
        part = np.zeros(NT, dtype=np.int64)
        for i0 in range(0, b, NT):
            i = i0 + tid
            part[i < b] += counts[i[i < b]]
            if defect == "index_first_256_counts":
                break
        base = int(part.sum())
        if b == B - 1:
            _store(bufs, "n_labels", 0, base + int(counts[b]))
        for i0 in range(0, L, NT):
            i = i0 + tid
            v = np.where(i < L, lab[b * L + np.minimum(i, L - 1)], IGNORE)
            on = (v != IGNORE).reshape(NT // WAVE, WAVE)
            s_wave = on.sum(axis=1)                          # popcount of each wave's ballot
            before = np.cumsum(on, axis=1) - on              # popcount of the ballot below the lane
            off = base + (0 if defect == "index_ignores_waves" else (np.cumsum(s_wave) - s_wave)[:, None])
            dest = (off + before)[on]
            _store(bufs, "label_rows", dest, (b * L + i)[on.reshape(-1)])
            _store(bufs, "label_ids", dest, v[on.reshape(-1)])
            base += int(s_wave.sum())


def corrupt_restated(cfg, inp, defect=None):
    bufs = new_buffers(corrupt_buffers(cfg))
    _corrupt_kernels(bufs, cfg["B"], cfg["N"], cfg["S"], inp["ids"], inp["lengths"], inp["u"], inp["rnd"], inp["family"],
                     cfg["desc"] == "given", cfg["index"] == "given", defect)
    return bufs


def corrupt_judge(cfg, inp, ref, out):
    return judge_buffers(corrupt_buffers(cfg), ref, out)


INDEX_PASS_NAMES = ("counts_loop_second_trip", "second_trip_adds_a_count", "zero_count_inside_the_prefix_sum", "labels_at_lanes_0_63_and_threads_0_255",
                    "full_wave_of_labels", "labels_behind_a_full_wave_in_its_trip", "labels_in_several_trips", "labels_in_several_waves_of_a_trip",
                    "index_exactly_full", "index_empty")


def corrupt_branch(cfg):
    inp = corrupt_inputs(cfg)
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    T, L, n2 = S + 1, S + N + 3, N + 2
    ref = _corrupt_plain(B, N, S, inp["ids"], inp["lengths"], inp["u"], inp["rnd"], inp["family"], inp["vocab"])
    lab, txt = ref["txt_labels"][0].reshape(B, L), ref["input_txt"][0].reshape(B, T)
    ln, raw = clamp_lengths(inp["lengths"], S), inp["lengths"]
    b = ["L=%d" % L, "trips=%d" % ((L + NT - 1) // NT), "N=%d" % N, "B=%d" % B, "draws_" + cfg["draws"], "family_" + cfg["family"],
         "desc_" + cfg["desc"], "index_" + cfg["index"], "n2<256" if n2 < NT else ("n2==256" if n2 == NT else "n2>256")]
    if B > NT + 1:
        b.append("counts_loop_second_trip")
        if ref["counts"][0][NT] > 0:
            b.append("second_trip_adds_a_count")
    for name, hit in (("len<0", raw < 0), ("len=0", raw == 0), ("len=1", raw == 1), ("len=S-1", raw == S - 1), ("len=S", raw == S), ("len>S", raw > S)):
        if hit.any():
            b.append(name)
    if B >= 3:
        for name, at in (("first", 0), ("middle", B // 2), ("last", B - 1)):
            if ln[at] == 0:
                b.append("zero_length_" + name)
    if (ref["counts"][0][:-1] == 0).any() and (ref["counts"][0][1:] > 0).any():
        b.append("zero_count_inside_the_prefix_sum")
    act = np.zeros((B, S), dtype=np.int64)
    for s in range(B):
        act[s, :ln[s]] = _mlm_action(inp["u"][s, :ln[s]], None)
        natural = int((act[s] > 0).sum())
        if ln[s] == 0:
            b.append("len0_no_forced_mask")
        elif natural == 0:
            b.append("forced_mask")
            b.append("forced_label_in_" + ("thread_0's_own_element" if n2 % NT == 0 else "another_thread's_element"))
        if ln[s] > 0 and natural == ln[s]:
            b.append("every_token_selected")
        on = np.nonzero(lab[s] != IGNORE)[0]
        if {0, WAVE - 1} <= set((on % WAVE).tolist()) and {0, NT - 1} <= set((on % NT).tolist()):
            b.append("labels_at_lanes_0_63_and_threads_0_255")
        for w0 in range(0, L - WAVE + 1, WAVE):
            if (lab[s, w0:w0 + WAVE] != IGNORE).all():
                b.append("full_wave_of_labels")
                if (lab[s, w0 + WAVE:(w0 // NT + 1) * NT] != IGNORE).any():
                    b.append("labels_behind_a_full_wave_in_its_trip")
        trips = set((on // NT).tolist())
        if len(trips) > 1:
            b.append("labels_in_several_trips")
        if any(len({int(i) // WAVE for i in on if i // NT == tr}) > 1 for tr in trips):
            b.append("labels_in_several_waves_of_a_trip")
        if natural == 1 and ln[s] > 1 and act[s, ln[s] - 1] > 0:
            b.append("only_the_last_token_selected")
    for name, a in (("mask", 1), ("random", 2), ("keep", 3), ("none", 0)):
        if (act == a).any():
            b.append("act_" + name)
    for v in RND_PLANTED:
        if ((act == 2) & (inp["rnd"] == v)).any():
            b.append("rnd=%d_used" % v)
    if cfg["draws"] == "edges" and ln.max() >= edge_draws().size:
        b.append("every_edge_draw_on_a_valid_token")
    if int(ref["n_labels"][0][0]) == B * S:
        b.append("index_exactly_full")
    if int(ref["n_labels"][0][0]) == 0:
        b.append("index_empty")
    assert (txt[np.arange(B), ln] == TOK_SEP).all()
    if cfg["index"] != "given":                              # names of the index pass: reached only where it runs
        b = [n for n in b if n not in INDEX_PASS_NAMES]
    return sorted(set(b))


# =====================================================================================================================
# mv_pack_plan
# =====================================================================================================================
PACK_B = (1, 2, 256, 257, 300)
PACK_L = (1, 255, 256, 257, 600)


def pack_cases():
    rows = [(1, 1, "mixed"), (1, 1, "zero"), (2, 255, "mixed"), (2, 256, "full"), (7, 257, "mixed"), (3, 600, "mixed"), (256, 5, "mixed"),
            (257, 3, "mixed"), (300, 257, "mixed"), (300, 1, "mixed"), (300, 4, "zero"), (300, 3, "full"), (5, 600, "full"), (2, 600, "zero"),
            (1, 256, "mixed"), (7, 255, "mixed"), (300, 6, "mixed")]
    return [dict(fam="pack", seed=s, B=B, L=L, vl=vl) for s, (B, L, vl) in enumerate(rows)]


def pack_inputs(cfg):
    rs = np.random.RandomState(7300 + cfg["seed"])
    B, L = cfg["B"], cfg["L"]
    desc = rs.randint(-9, 4000, size=(B, 3)).astype(I32)                # columns 0 and 1 are not the kernel's business
    if cfg["vl"] == "zero":
        desc[:, 2] = [(0, -4)[b % 2] for b in range(B)]
    elif cfg["vl"] == "full":
        desc[:, 2] = [(L, L + 9)[b % 2] for b in range(B)]
    else:
        cls = [-5, 0, 1, L - 1, L, L + 7]
        desc[:, 2] = [cls[(b + cfg["seed"]) % 6] for b in rs.permutation(B)] if B > 1 else cls[cfg["seed"] % 6]
        if B == 300:
            desc[256, 2] = L                                            # the first count the second trip of the prefix loop adds
    return dict(desc=desc)


def pack_buffers(cfg):
    B, L = cfg["B"], cfg["L"]
    return dict(cu=(I32, B + 1), rowmap=(I32, B * L), inv=(I32, B * L))


def _pack_plain(B, L, desc):
    vl = np.clip(desc[:, 2].astype(np.int64), 0, L)
    cu = np.concatenate([[0], np.cumsum(vl)])
    rowmap, inv = [], np.full(B * L, -1, dtype=I32)
    for b in range(B):
        for p in range(int(vl[b])):
            inv[b * L + p] = len(rowmap)
            rowmap.append(b * L + p)
    assert len(rowmap) == cu[B]
    return dict(cu=_all(cu, I32), rowmap=_head(rowmap, B * L, I32), inv=_all(inv, I32))


def pack_reference(cfg, inp):
    return _pack_plain(cfg["B"], cfg["L"], inp["desc"])


def _pack_kernel(bufs, B, L, desc, defect):
    tid = np.arange(NT)
    d2 = desc[:, 2].astype(np.int64)
    clamp = (lambda v: v) if defect == "no_clamp" else (lambda v: np.minimum(np.maximum(v, 0), L))
    for b in range(B):
        part = np.zeros(NT, dtype=np.int64)
        for i0 in range(0, b, NT):
            i = i0 + tid
            part[i < b] += clamp(d2[i[i < b]])
        base = int(part.sum())
        vl = int(clamp(d2[b]))
        _store(bufs, "cu", b, base)
        if b == B - 1:
            _store(bufs, "cu", B, base + vl)
        for p0 in range(0, L, NT):
            p = p0 + tid
            p = p[p < L]
            keep = p < vl
            m = np.ones_like(keep) if defect == "rowmap_for_dropped" else keep
            _store(bufs, "rowmap", base + p[m], b * L + p[m])
            _store(bufs, "inv", b * L + p, np.where(keep, base + p, -1))


def pack_restated(cfg, inp, defect=None):
    bufs = new_buffers(pack_buffers(cfg))
    _pack_kernel(bufs, cfg["B"], cfg["L"], inp["desc"], defect)
    return bufs


def pack_judge(cfg, inp, ref, out):
    return judge_buffers(pack_buffers(cfg), ref, out)


def pack_branch(cfg):
    B, L = cfg["B"], cfg["L"]
    v = pack_inputs(cfg)["desc"][:, 2]
    b = ["B=%d" % B, "L=%d" % L, "vl_" + cfg["vl"], "prefix_trips=%d" % ((max(B - 1, 0) + NT - 1) // NT), "row_trips=%d" % ((L + NT - 1) // NT)]
    for name, hit in (("vl<0", v < 0), ("vl=0", v == 0), ("vl=1", v == 1), ("vl=L-1", v == L - 1), ("vl=L", v == L), ("vl>L", v > L)):
        if hit.any():
            b.append(name)
    if sum(bool(h.any()) for h in (v < 0, v > L, (v > 0) & (v < L))) >= 2:
        b.append("classes_mixed_in_a_batch")
    total = int(np.clip(v, 0, L).sum())
    b.append("cu[B]=0" if total == 0 else ("cu[B]=B*L" if total == B * L else "cu[B]_between"))
    if B > 1 and np.clip(v[-1], 0, L) < L:
        b.append("last_sample_drops_positions")
    if B > NT + 1 and np.clip(v[NT], 0, L) > 0:
        b.append("second_trip_adds_a_count")
    return b


# =====================================================================================================================
# mv_tail_perm
# =====================================================================================================================
TAIL_ROWS = {
    "one_0": (0,), "one_1": (1,), "one_64": (64,), "one_2048": (2048,), "all_0": (0, 0, 0, 0, 0),
    "five_wave": (63, 64, 65, 0, 1), "five_block": (256, 0, 257, 1, 65), "five_cap": (2048, 0, 257, 256, 1),
    "cycle300": tuple((0, 1, 63, 64, 65, 256, 257, 5)[b % 8] for b in range(300)),
}
TAIL_NSEL = (1, 255, 256, 257, "over")
TAIL_SEL = ("shuffled", "dups", "none_in_one", "all_in_one", "offsets", "minus1", "beyond")


def tail_cases():
    rows = [("one_1", 1, 1, "shuffled"), ("one_1", 1, 255, "dups"), ("one_0", 1, 1, "minus1"), ("one_0", 7, 256, "beyond"), ("one_64", 64, "over", "dups"),
            ("one_64", 64, 257, "minus1"), ("one_2048", 2048, 257, "shuffled"), ("one_2048", 2048, 256, "offsets"), ("one_2048", 2048, "over", "all_in_one"),
            ("all_0", 3, 255, "beyond"), ("all_0", 3, 1, "beyond"), ("five_wave", 65, 255, "offsets"), ("five_wave", 65, 257, "all_in_one"),
            ("five_wave", 100, "over", "minus1"), ("five_wave", 65, 1, "shuffled"), ("five_block", 257, 256, "none_in_one"),
            ("five_block", 257, 257, "all_in_one"), ("five_block", 300, "over", "beyond"), ("five_block", 257, 255, "offsets"),
            ("five_cap", 2048, 257, "none_in_one"), ("five_cap", 2048, "over", "minus1"), ("five_cap", 2048, 256, "offsets"),
            ("cycle300", 257, 257, "shuffled"), ("cycle300", 257, "over", "beyond"), ("cycle300", 300, 256, "offsets"), ("cycle300", 257, 255, "dups"),
            ("cycle300", 257, "over", "minus1"), ("cycle300", 257, 257, "all_in_one")]
    return [dict(fam="tail", seed=s, rows=r, L=L, n_sel=n, sel=k) for s, (r, L, n, k) in enumerate(rows)]


def tail_inputs(cfg):
    rs = np.random.RandomState(7400 + cfg["seed"])
    rows = TAIL_ROWS[cfg["rows"]]
    cu = np.concatenate([[0], np.cumsum(rows)]).astype(I32)
    B, M = len(rows), int(cu[-1])
    n_sel = M + 9 if cfg["n_sel"] == "over" else cfg["n_sel"]
    kind = cfg["sel"]
    sizes = sorted(((n, b) for b, n in enumerate(rows) if n > 0), reverse=True)
    special, excluded, filler = [], -1, None
    if kind == "offsets":
        for b, n in enumerate(rows):
            special += [int(cu[b]) + o for o in sorted({0, 63, 64, n - 1}) if 0 <= o < n]
    elif kind == "all_in_one":
        fit = [(n, b) for n, b in sizes if n <= n_sel]
        if fit:
            special = list(range(int(cu[fit[0][1]]), int(cu[fit[0][1] + 1])))
    elif kind == "none_in_one" and sizes:
        excluded = sizes[0][1]
    elif kind == "minus1":
        special, filler = [-1, -1, -5], -1
    elif kind == "beyond":
        special, filler = [M, M + 5, 2 ** 31 - 1], M + 1
    pool = [int(r) for r in rs.permutation(M) if not (excluded >= 0 and cu[excluded] <= r < cu[excluded + 1])]
    if kind == "dups" and pool:
        special = [pool[j % len(pool)] for j in (0, 0, 0, 1, 1)]
    sel = (special + [r for r in pool if r not in set(special)])[:n_sel]
    while len(sel) < n_sel:                                  # more entries than rows: repeats, or entries in no sample
        sel.append(filler if filler is not None else (sel[int(rs.randint(len(sel)))] if sel else -1))
    sel = np.array(sel, dtype=np.int64)[rs.permutation(n_sel)]
    return dict(cu=cu, sel=sel.astype(I32), B=B, M=M, n_sel=n_sel)


TAIL_SLACK = 32               # elements of perm / newpos behind cu[B]: "not written from cu[B] on" needs somewhere to look


def tail_buffers(cfg, inp):
    return dict(perm=(I32, inp["M"] + TAIL_SLACK), newpos=(I32, inp["M"] + TAIL_SLACK), qlim=(I32, inp["B"]), sel_new=(I32, inp["n_sel"]))


def _tail_plain(cu, sel, slack=TAIL_SLACK):
    B, M = len(cu) - 1, int(cu[-1])
    chosen = set(int(s) for s in sel)
    perm, qlim = [], []
    for b in range(B):
        rows = list(range(int(cu[b]), int(cu[b + 1])))
        perm += sorted(rows, key=lambda r: r not in chosen)                  # stable: the consumed rows first, each part ascending
        qlim.append(sum(r in chosen for r in rows))
    newpos = np.zeros(M, dtype=np.int64)
    newpos[np.array(perm, dtype=np.int64)] = np.arange(M)
    assert sorted(perm) == list(range(M))
    sel_new = [int(newpos[s]) if 0 <= s < M else -1 for s in sel.tolist()]
    return dict(perm=_head(perm, M + slack, I32), newpos=_head(newpos, M + slack, I32), qlim=_all(qlim, I32), sel_new=_all(sel_new, I32))


def tail_reference(cfg, inp):
    return _tail_plain(inp["cu"], inp["sel"])


def _tail_kernel(bufs, cu, sel, defect):
    B, n_sel = len(cu) - 1, len(sel)
    tid, lane = np.arange(NT), np.arange(WAVE)
    sel = sel.astype(np.int64)
    for b in range(B):
        lo, n = int(cu[b]), int(cu[b + 1]) - int(cu[b])
        assert n <= TP_MAXL
        flag = np.zeros(TP_MAXL, dtype=np.uint8)
        dup = 0
        for i0 in range(0, n_sel, NT):
            i = i0 + tid
            r = sel[i[i < n_sel]] - lo
            r = r[(r >= 0) & (r < n)]
            flag[r] = 1
            dup += r.size
        pos = 0
        newpos = {}
        for ps in range(2):
            for c in range(0, n, WAVE):
                r = c + lane
                f = (r < n) & ((flag[np.minimum(r, TP_MAXL - 1)] != 0) == ((ps == 0) != (defect == "unselected_first")))
                p = pos + np.cumsum(f) - f
                _store(bufs, "perm", lo + p[f], lo + r[f])
                _store(bufs, "newpos", lo + r[f], lo + p[f])
                newpos.update(zip((lo + r[f]).tolist(), (lo + p[f]).tolist()))
                pos += int(f.sum())
            if ps == 0:
                _store(bufs, "qlim", b, dup if defect == "qlim_counts_duplicates" else pos)
        for i0 in range(0, n_sel, NT):
            i = i0 + tid
            i = i[i < n_sel]
            s = sel[i]
            inside = (s >= lo) & (s - lo < n)
            _store(bufs, "sel_new", i[inside], [newpos[int(v)] for v in s[inside]])
            if defect != "sel_new_unwritten":
                nowhere = ((b == 0) & (s < lo)) | ((b == B - 1) & (s >= lo + n))
                _store(bufs, "sel_new", i[nowhere], -1)


def tail_restated(cfg, inp, defect=None):
    bufs = new_buffers(tail_buffers(cfg, inp))
    _tail_kernel(bufs, inp["cu"], inp["sel"], defect)
    return bufs


def tail_judge(cfg, inp, ref, out):
    ok, what = judge_buffers(tail_buffers(cfg, inp), ref, out)
    if ok:                                                   # what the contract says in words, on the output itself
        M = inp["M"]
        perm, newpos = out["perm"][GUARD:GUARD + M], out["newpos"][GUARD:GUARD + M]
        if not (np.array_equal(np.sort(perm), np.arange(M)) and np.array_equal(perm[newpos], np.arange(M))):
            ok, what = False, "perm and newpos are not inverse permutations of 0..cu[B]-1"
    return ok, what


def tail_branch(cfg):
    inp = tail_inputs(cfg)
    cu, sel, B, M = inp["cu"], inp["sel"].astype(np.int64), inp["B"], inp["M"]
    rows = np.diff(cu)
    b = ["B=%d" % B, "n_sel=%s" % ("over" if cfg["n_sel"] == "over" else inp["n_sel"]), "sel_trips=%d" % ((inp["n_sel"] + NT - 1) // NT)]
    b += ["rows=%d" % n for n in set(rows.tolist()) if n in (0, 1, 63, 64, 65, 256, 257, 2048)]
    if cfg["L"] == TP_MAXL:
        b.append("L=2048")
    if inp["n_sel"] > M:
        b.append("n_sel>cu[B]")
    if M == 0:
        b.append("cu[B]=0")
    inside = sel[(sel >= 0) & (sel < M)]
    if len(set(inside.tolist())) < inside.size:
        b.append("sel_duplicates")
    if inside.size > 1 and (np.diff(inside) < 0).any():
        b.append("sel_shuffled")
    if (sel == -1).any():
        b.append("sel_minus1")
    if (sel < -1).any():
        b.append("sel_below_minus1")
    if (sel >= M).any():
        b.append("sel_beyond_cu[B]")
    if (sel == M).any():
        b.append("sel_equals_cu[B]")
    chosen = set(inside.tolist())
    for s in range(B):
        lo, n = int(cu[s]), int(rows[s])
        k = sum(r in chosen for r in range(lo, lo + n))
        if n > 0 and k == 0:
            b.append("sample_with_no_selected_row")
        if n > 0 and k == n:
            b.append("sample_with_every_row_selected")
        if 0 < k < n:
            b.append("sample_partly_selected")
        for o in (0, 63, 64):
            if o < n and lo + o in chosen:
                b.append("sel_offset_%d" % o)
        if n > 1 and lo + n - 1 in chosen:
            b.append("sel_offset_n-1")
        if n > WAVE and 0 < k < n:
            b.append("partition_over_several_chunks")
    return sorted(set(b))


# =====================================================================================================================
# the chain: draws -> corrupt -> desc -> pack_plan -> sel = cat(inv[label_rows], cu[:B]) -> tail_perm
# =====================================================================================================================
CHAIN_SHAPES = ((5, 6, 40), (9, 36, 217))


def chain_cases():
    out = []
    for s, ((B, N, S), extra) in enumerate([(sh, ex) for sh in CHAIN_SHAPES for ex in ("none", "dropped")]):
        out.append(dict(fam="chain", seed=s, B=B, N=N, S=S, extra=extra, key=KEY_HI + 977 * s))
    return out


def chain_inputs(cfg):
    rs = np.random.RandomState(7500 + cfg["seed"])
    B, S = cfg["B"], cfg["S"]
    lengths = rs.randint(2, S, size=B).astype(I32)
    lengths[1], lengths[B - 2] = 1, S
    lengths[2] = 3                                           # three tokens: most keys select none of them
    ids = rs.randint(1000, VOCAB, size=(B, S)).astype(I64)
    fams = [("full", "1d")[int(v)] for v in rs.randint(0, 2, size=B)]
    fams[0], fams[1] = "full", "1d"
    return dict(ids=ids, lengths=lengths, fams=fams, family=np.array([FAMILY_ID[f] for f in fams], dtype=I32), key=cfg["key"], vocab=VOCAB)


def chain_tail_rows(cfg, label_rows, n_labels):
    """the tail_rows the engine is handed: the labelled rows -- and, for `dropped`, a padding position of the one-token sample"""
    L = cfg["S"] + cfg["N"] + 3
    rows = [int(r) for r in label_rows[:n_labels]]
    return rows + ([1 * L + L - 1] if cfg["extra"] == "dropped" else [])


def _chain_sizes(cfg, n_labels, M):
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    n_sel = n_labels + (1 if cfg["extra"] == "dropped" else 0) + B
    specs = dict(u=(F32, B * S), rnd=(I32, B * S))
    specs.update(corrupt_buffers(cfg))
    specs.update(cu=(I32, B + 1), rowmap=(I32, B * (S + N + 3)), inv=(I32, B * (S + N + 3)))
    specs.update(perm=(I32, M + TAIL_SLACK), newpos=(I32, M + TAIL_SLACK), qlim=(I32, B), sel_new=(I32, n_sel))
    return specs


def chain_buffers(cfg, ref):
    return _chain_sizes(cfg, int(ref["n_labels"][0][0]), int(ref["cu"][0][-1]))


def chain_reference(cfg, inp):
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    L = S + N + 3
    u, rnd = draw_stream(inp["key"], B, S, inp["vocab"])
    ref = dict(u=_all(u, F32), rnd=_all(rnd, I32))
    ref.update(_corrupt_plain(B, N, S, inp["ids"], inp["lengths"], u, rnd, inp["family"], inp["vocab"]))
    desc = ref["desc"][0].reshape(B, 3)
    ref.update(_pack_plain(B, L, desc))
    cu, inv = ref["cu"][0], ref["inv"][0]
    n = int(ref["n_labels"][0][0])
    sel = np.array([inv[r] for r in chain_tail_rows(cfg, ref["label_rows"][0], n)] + cu[:B].tolist(), dtype=I32)
    ref.update(_tail_plain(cu, sel))
    ref["sel"] = sel
    return ref


def chain_restated(cfg, inp, defect=None):
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    L = S + N + 3
    stage = dict(u=(F32, B * S), rnd=(I32, B * S))
    stage.update(corrupt_buffers(cfg))
    stage.update(cu=(I32, B + 1), rowmap=(I32, B * L), inv=(I32, B * L))
    bufs = new_buffers(stage)
    _draws_kernel(bufs, ("u", "rnd"), inp["key"], B, S, inp["vocab"], defect)
    _corrupt_kernels(bufs, B, N, S, inp["ids"], inp["lengths"], _body(bufs, "u").reshape(B, S), _body(bufs, "rnd").reshape(B, S),
                     inp["family"], True, True, defect)
    _pack_kernel(bufs, B, L, _body(bufs, "desc").reshape(B, 3), defect)
    n, cu = int(_body(bufs, "n_labels")[0]), _body(bufs, "cu")
    n = min(max(n, 0), B * S)
    inv = _body(bufs, "inv")
    sel = np.array([inv[r] for r in chain_tail_rows(cfg, _body(bufs, "label_rows"), n)] + cu[:B].tolist(), dtype=I32)
    M = min(max(int(cu[B]), 0), B * L)
    bufs.update(new_buffers(dict(perm=(I32, M + TAIL_SLACK), newpos=(I32, M + TAIL_SLACK), qlim=(I32, B), sel_new=(I32, sel.size))))
    _tail_kernel(bufs, cu, sel, defect)
    bufs["sel"] = sel
    return bufs


def chain_twins(cfg, inp, ref):
    """the project's host twins on the chain's intermediate results -> list of disagreements"""
    import torch
    from medvill_amd import data
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    L = S + N + 3
    what = []
    n = int(ref["n_labels"][0][0])
    rows, lids = data.label_index(torch.from_numpy(ref["txt_labels"][0].reshape(B, L)))
    if rows.dtype != torch.int32 or not (np.array_equal(rows.numpy(), ref["label_rows"][0][:n]) and np.array_equal(lids.numpy(), ref["label_ids"][0][:n])):
        what.append("data.label_index")
    md = data.MaskDesc.make(inp["fams"], N, S, torch.from_numpy(ref["n_ids"][0].copy()))
    if md.L != L or not np.array_equal(md.desc.numpy().reshape(-1), ref["desc"][0]):
        what.append("data.MaskDesc.make")
    hd = md.host_desc()
    if int(hd[:, 2].clamp(0, L).sum()) != int(ref["cu"][0][B]):
        what.append("the engine's M")
    return what


def chain_judge(cfg, inp, ref, out):
    ok, what = judge_buffers(chain_buffers(cfg, ref), ref, out)
    if ok and not np.array_equal(np.asarray(out["sel"]), ref["sel"]):
        ok, what = False, "sel"
    twins = chain_twins(cfg, inp, ref)
    if twins:
        ok, what = False, (what + "; " if what else "") + "host twins disagree with the reference: " + ", ".join(twins)
    return ok, what


def chain_branch(cfg):
    inp = chain_inputs(cfg)
    ref = chain_reference(cfg, inp)
    B, S = cfg["B"], cfg["S"]
    ln = clamp_lengths(inp["lengths"], S)
    u = ref["u"][0].reshape(B, S)
    b = ["shape=%dx%dx%d" % (cfg["B"], cfg["N"], cfg["S"]), "extra_" + cfg["extra"]] + ["family_" + f for f in set(inp["fams"])]
    if (ln == 1).any():
        b.append("len=1")
    if (ln == S).any():
        b.append("len=S")
    if any(not (u[s, :ln[s]].astype(np.float64) < P_SELECT).any() for s in range(B)):
        b.append("sample_without_natural_selection")
    if (ref["sel"] == -1).any():
        b.append("sel_names_a_dropped_position")
    if (ref["sel_new"][0] == -1).any():
        b.append("sel_new=-1")
    if (ref["inv"][0] == -1).any():
        b.append("positions_dropped")
    return sorted(set(b))


# =====================================================================================================================
# census, defects
# =====================================================================================================================
FAMILIES = {
    "draws": (draws_cases, draws_branch, draws_inputs, draws_reference, draws_restated, draws_judge),
    "corrupt": (corrupt_cases, corrupt_branch, corrupt_inputs, corrupt_reference, corrupt_restated, corrupt_judge),
    "pack": (pack_cases, pack_branch, pack_inputs, pack_reference, pack_restated, pack_judge),
    "tail": (tail_cases, tail_branch, tail_inputs, tail_reference, tail_restated, tail_judge),
    "chain": (chain_cases, chain_branch, chain_inputs, chain_reference, chain_restated, chain_judge),
}

DEFECTS = {
    "draws": ["rnd_mod", "u_low24", "index_transposed"],
    "corrupt": ["le_0.15", "le_0.8", "forced_when_len0", "forced_labels_corrupted", "sep_late", "label_offset_N+1", "index_ignores_waves",
                "index_first_256_counts"],
    "pack": ["no_clamp", "rowmap_for_dropped"],
    "tail": ["unselected_first", "qlim_counts_duplicates", "sel_new_unwritten"],
    "chain": ["sel_new_unwritten"],
}


_MEMO = {}


def _memo(kind, cfg, make):
    key = (kind, case_id(cfg))
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def branches(cfg):
    """the branch names of a case (computed once per case: they need its reference)"""
    return _memo("branch", cfg, lambda: frozenset(FAMILIES[cfg["fam"]][1](cfg)))


def census(fam, drop=None):
    """branch name -> number of cases of the family that reach it (`drop`: without the case of that index)"""
    count = {}
    for k, c in enumerate(FAMILIES[fam][0]()):
        if k != drop:
            for name in branches(c):
                count[name] = count.get(name, 0) + 1
    return count


def run_restated(cfg, defect=None):
    """a case through its restatement and the judgement, as the GPU file runs it through the kernels -> (ok, what).  The inputs and the
    reference of a case are made once and shared by every defect; nothing writes to them."""
    _, _, inputs, reference, restated, judge = FAMILIES[cfg["fam"]]
    inp = _memo("inputs", cfg, lambda: inputs(cfg))
    ref = _memo("reference", cfg, lambda: reference(cfg, inp))
    return judge(cfg, inp, ref, restated(cfg, inp, defect))
