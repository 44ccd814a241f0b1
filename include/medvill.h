/*
 * medvill.h -- C ABI of the MI355X (gfx950) hot-path library for MedViLL / CXRBERT
 * cross-modal BERT pretraining (libmedvill_hip.so).
 *
 * The reference (reonaledo/Multi-modality-Self-supervision) is pure Python and has no
 * FFI layer: its boundary is the Python object protocol
 *     CXRBERT(config, args).forward(cls_tok, input_txt, attn_mask, segment, input_img, sep_tok)
 *         -> (mlm_logits[B,L,V], itm_logits[B,2])          models/cxrbert_origin.py:132-149
 *     CXRBERT_Trainer(args, train_dataloader, test_dataloader).train(epoch) / .save(epoch, path)
 *                                                            models/train_origin.py:19-20,70,254
 * which `multi-modality-self-supervision_amd/` mirrors in Python.  Underneath that
 * mirror every piece of arithmetic goes through the entry points below; each one
 * names the reference code whose work it replaces.  (INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; all data pointers are DEVICE pointers owned
 *     by the caller (torch's allocator); no allocation inside, workspaces are passed in.
 *   - every call takes the hipStream_t to enqueue on (as void*) and never synchronises.
 *   - return 0 = ok; negative = invalid argument / unsupported shape (MV_E_*);
 *     positive = hipError_t of a failed launch.  Nothing throws.
 *   - re-entrant, no global mutable state: which kernel serves a call follows from the call's arguments alone.  (The kernel-forcing
 *     knobs that tests and timing experiments use exist only in libmedvill_hip_dbg.so: include/medvill_debug.h.)
 *   - dtype: MV_F32 = exact fp32 path (plain VALU kernels; parity at 1e-3 and below),
 *            MV_BF16 / MV_F16 = 16-bit storage, fp32 accumulate, MFMA kernels (the fast path).
 *   - matrices are row-major; "ld*" are leading dimensions in ELEMENTS.
 */
#ifndef MEDVILL_H_
#define MEDVILL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MV_ABI_VERSION 6

/* MV_F16 is the encoding of the 16-bit path (weights' f16 shadow, stored activations, gradients): 11 significand bits
 * instead of bf16's 8 at the same MFMA rate.  At BERT-base depth bf16-encoded forward operands cannot meet the 1e-2 logit
 * tolerance (the weight rounding alone gives 1.4e-2, profiles/r02_bf16_error.txt).  Gradients in f16 need a LOSS SCALE
 * (f16 has 5 exponent bits): the loss gradients are multiplied by S where they enter the 16-bit chain (mv_ce_fwd_bwd),
 * every kernel that writes an f32 PARAMETER gradient multiplies by 1/S again (grad_unscale_dev of mv_gemm / mv_colsum /
 * mv_layernorm_bwd / mv_embed_bwd), so the flat f32 gradient always holds true values; S lives on the device and is
 * adapted by mv_scaler_update from mv_count_nonfinite's overflow count (an overflowed step is skipped by mv_adamw_step).
 * The round-2 form remains available: f16 forward operands with MV_BF16 gradient operands, for which kernels that produce
 * a forward activation write it twice from one accumulator (C3 / y_bf16 / ctx_bf16 / x0_bf16 below). */
enum { MV_F32 = 0, MV_BF16 = 1, MV_F16 = 2 };

enum {
  MV_OK = 0,
  MV_E_ARG = -1,      /* null pointer / non-positive size */
  MV_E_SHAPE = -2,    /* shape or alignment the kernels do not support */
  MV_E_DTYPE = -3,
  MV_E_WORKSPACE = -4, /* workspace too small */
  MV_E_NO_RCCL = -5,   /* mv_comm_*: librccl could not be loaded at run time */
  MV_E_COMM_BASE = -1000 /* mv_comm_*: a failed RCCL call returns MV_E_COMM_BASE - ncclResult_t (-1001, -1002, ...): negative like every
                            MV_E_* code, disjoint from hipError_t (positive, some of them above 1000) */
};

/* GEMM epilogues (mv_gemm `epi`) */
enum {
  MV_EPI_NONE = 0,      /* C = A.B                                                        */
  MV_EPI_BIAS = 1,      /* C = A.B + bias[n]                                              */
  MV_EPI_BIAS_GELU = 2, /* Z = A.B + bias -> C2 (pre-activation, kept for backward);
                           C = gelu_erf(Z)          cxrbert_origin.py:176-181 / HF BertIntermediate */
  MV_EPI_BIAS_RES = 3,  /* C = A.B + bias[n] + R[m,n]   (HF BertSelfOutput / BertOutput before LayerNorm) */
  MV_EPI_DGELU = 4,     /* C = (A.B) * gelu_erf'(R[m,n])   (backward of MV_EPI_BIAS_GELU; R = saved Z)  */
  MV_EPI_RES = 5,       /* C = A.B + R[m,n]             (backward: add the residual-branch gradient)    */
  MV_EPI_BIAS_TANH = 6, /* C = tanh(A.B + bias)         HF BertPooler, cxrbert_origin.py:130            */
  MV_EPI_BIAS_GELU_D = 7, /* Z = A.B + bias; C = gelu_erf(Z); C2 = gelu_erf'(Z): the derivative shares the forward's exp and
                             reciprocal, so the backward GEMM only multiplies (MV_EPI_MUL) and Z itself is never stored */
  MV_EPI_MUL = 8,       /* C = (A.B) * R[m,n]           (backward of MV_EPI_BIAS_GELU_D; R = saved gelu')  */
  MV_EPI_BIAS_RELU = 9,      /* C = max(A.B + bias[n], 0)            convolution + folded BatchNorm + ReLU (region encoder, eval()) */
  MV_EPI_BIAS_RES_RELU = 10  /* C = max(A.B + bias[n] + R[m,n], 0)   ... + the bottleneck's identity branch                          */
};

int mv_abi_version(void);
const char* mv_build_info(void);
/* A HIP stream whose kernels run only on the CUs of `mask_words` (n_words x 32 bits; hipExtStreamCreateWithCUMask; on a multi-XCD
 * device bit i is CU i / n_xcd of XCD i % n_xcd): lets a host partition the chip between the streams of a step. */
int mv_stream_create_cumask(const uint32_t* mask_words, int n_words, void** stream_out);
int mv_stream_destroy(void* stream);

/* ---- dense projections --------------------------------------------------------------------
 * Replaces every nn.Linear on the path and its autograd backward:
 *   cxrbert_origin.py:16,24 (image projection), HF BertSelfAttention/BertSelfOutput/
 *   BertIntermediate/BertOutput/BertPooler (call sites cxrbert_origin.py:72-73,126-130),
 *   cxrbert_origin.py:214,228-237 (MLM transform + tied decoder), :170-173 (ITM).
 * C[M,N] = epi( opA(A)[M,K] . opB(B)[K,N] ):
 *   ta = 0: A stored [M,K] (lda >= K);  ta = 1: A stored [K,M] (lda >= M)
 *   tb = 0: B stored [N,K] (ldb >= K) -- an nn.Linear weight;  tb = 1: B stored [K,N] (ldb >= N)
 * so  y = x.W^T            is (ta=0, tb=0, A=x,  B=W)
 *     dx = dy.W            is (ta=0, tb=1, A=dy, B=W)
 *     dW = dy^T.x          is (ta=1, tb=1, A=dy, B=x)
 * dtype applies to A and B (MV_F16 for every form but ta = 1, tb = 0); c_dtype to C (and C2); r_dtype to R; bias is always f32.
 * C3 (nullable, leading dimension ldc3): a second copy of C in the 16-bit encoding c3_dtype (see MV_F16 above).
 * 16-bit operands need 16-byte aligned bases and lda, ldb multiples of 8; a contraction length
 * K that is not a multiple of 8 is allowed only when the k-contiguous operand's rows are
 * zero-padded up to the next multiple of 8.
 * splitk = 0: let the library pick (up to 32 slices on the 256-row kernels, as many as ws holds; up to 16 on the 128x128
 * kernel, which takes its whole wish or, when ws is smaller than that, 1; without ws 1 is used).
 * splitk > 1: the K range is cut in `splitk` slices whose partial tiles go to `ws`
 * (>= splitk*M*N floats) and are summed by a second kernel; only with MV_EPI_NONE and an f32 C.
 * accumulate != 0: C += result (f32 C, MV_EPI_NONE only).
 * p_drop > 0 (MV_EPI_BIAS_RES only, N % 4 == 0): C = dropout(A.B + bias) + R -- the hidden-state dropout
 * of HF BertSelfOutput / BertOutput; mask = mv_dropout_mask(p_drop, drop_key) over index m*N + n.
 * alpha_dev (nullable; MV_EPI_NONE with an f32 C only): C = *alpha_dev * (A.B) -- the weight gradients of the f16-gradient
 * path are un-scaled (1 / loss scale, read from the device) where they are written.
 * colsum_part (nullable): f32 [2*ceil(M/256)][N] -- the kernel also writes the column sums of C, one partial row per 128-row
 * tile half, so a bias gradient needs no second pass over C (fold with mv_colsum_partials).  Only where the 256x256 MFMA
 * kernel runs with 16-bit C, N % 256 == 0, 16-byte aligned outputs, no split-K (else MV_E_SHAPE: use mv_colsum).  */
int mv_gemm(int dtype, int ta, int tb, int M, int N, int K,
            const void* A, int lda, const void* B, int ldb,
            void* C, int ldc, int c_dtype,
            const float* bias, int epi,
            const void* R, int ldr, int r_dtype,
            void* C2, int ldc2,
            void* C3, int ldc3, int c3_dtype,
            int splitk, float* ws, size_t ws_bytes, int accumulate,
            float p_drop, unsigned long long drop_key, const float* alpha_dev, float* colsum_part, void* stream);

/* Split-K workspace sizes (SURVEY 8b's mv_workspace_bytes): what a host needs to allocate without reading the dispatch code.
 *   mv_gemm_workspace_bytes  bytes of `ws` with which mv_gemm(splitk = 0) takes the split-K choice it prefers for this product
 *                            (slabs x M x N x 4; 0 = this call never splits: f32 data, a wide / large product, K < 2048).  A smaller
 *                            workspace is legal: the 256-row kernels then take as many slabs as fit, the 128x128 kernel does
 *                            not split (one slab).
 *   mv_workspace_bytes       the largest such workspace any mv_gemm call of a pretraining step asks for at this geometry (weight
 *                            gradients of the four encoder projections, of the MLM transform and of the image projection over
 *                            `max_rows` / `max_label_rows` / `max_regions` rows; the tied decoder's input gradient over the
 *                            vocabulary).  One workspace PER STREAM that issues split-K products concurrently.  Pure functions. */
size_t mv_gemm_workspace_bytes(int dtype, int ta, int tb, int M, int N, int K);
size_t mv_workspace_bytes(int hidden, int intermediate, int vocab, int img_hidden, int max_rows, int max_label_rows, int max_regions);

/* ---- grouped weight gradients ---------------------------------------------------------------
 * Many independent products C_i[No_i, Ko_i] (+)= [*alpha_dev] * A_i[rows_i, No_i]^T . B_i[rows_i, Ko_i]  (the dW = dy^T.x form of
 * mv_gemm: 16-bit A and B of one encoding, f32 C) in ONE persistent launch over full contractions: a single product of a layer has
 * too few 256 x 256 tiles for the chip and needs split-K slabs, the products of all layers together do not.  Only the tiles that do
 * not fill a last round of blocks are cut along K (slabs in `ws`, folded by one reduction launch).
 *   mv_gemm_grouped_table_bytes      size of the table for `count` problems (0 for count <= 0).
 *   mv_gemm_grouped_fill             validates `problems` (host array) and writes the table into HOST memory `table_host`; n_blocks
 *                                    = blocks the launch will use (0: one per CU of the current device).  Pure host arithmetic.
 *                                    The caller keeps a copy of the table in device memory and refreshes it only when a problem
 *                                    changed: a launch copies nothing from the host.
 *   mv_gemm_grouped_workspace_bytes  bytes of `ws` the launch of this (host) table needs (0: nothing is split).
 *   mv_gemm_grouped_decode           launch unit -> out[7] = {problem, m0, n0, kbeg, kend, slice (-1: unsplit), flat tile}: the
 *                                    map the kernel itself uses, for hosts and tests that want to inspect a plan.
 *   mv_gemm_grouped_tn               the launch.  table_host: what mv_gemm_grouped_fill wrote (re-validated here; it decides the
 *                                    grid); table_dev: its device copy, which is all the kernels read.  The library cannot read
 *                                    device memory on the host, so table_dev is NOT checked: it must hold, when the launch runs
 *                                    on `stream`, the very bytes of table_host (all mv_gemm_grouped_table_bytes(count) of them).
 *                                    A stale or foreign device copy makes the kernels read and write through its pointers.
 *                                    accumulate / alpha_dev as in mv_gemm.
 * Per problem: A, B, C non-null, sizes positive (MV_E_ARG); A and B 16-byte aligned, C 4-byte aligned, lda and ldb multiples of
 * 8, lda >= No, ldb >= Ko, ldc >= Ko, every operand below 2 GiB, at most 256 problems (MV_E_SHAPE); dtype MV_BF16 or MV_F16
 * (MV_E_DTYPE); a null or foreign table, count <= 0 (MV_E_ARG); a table buffer or `ws` that is too small (MV_E_WORKSPACE).  A call
 * that fails launches nothing.  */
typedef struct mv_group_problem {
  const void* A; const void* B; void* C;
  int lda, ldb, ldc;
  int No, Ko, rows;
} mv_group_problem;
size_t mv_gemm_grouped_table_bytes(int count);
int mv_gemm_grouped_fill(int dtype, int count, const mv_group_problem* problems, int n_blocks, void* table_host, size_t table_bytes);
size_t mv_gemm_grouped_workspace_bytes(const void* table_host);
int mv_gemm_grouped_decode(const void* table_host, int unit, int* out);
int mv_gemm_grouped_tn(int dtype, int count, const void* table_host, const void* table_dev, float* ws, size_t ws_bytes,
                       int accumulate, const float* alpha_dev, void* stream);

/* ---- attention masks ----------------------------------------------------------------------
 * Replaces CXRBertEncoder.get_extended_attn_mask (cxrbert_origin.py:75-85): instead of an
 * fp16 additive [B,1,L,L] tensor the int64 0/1 mask the Dataset built
 * (data/dataset_origin.py:138-176) is packed once per batch into
 *   bits     uint32 [B, L, W]   W = ceil(L/32); bit (j&31) of word j>>5 = mask[b,i,j]
 *   tileinfo uint8  [B, TQ, TK] TQ = TK = ceil(L/64); per 64x64 tile: 0 = every entry masked and
 *                               every query row of the tile sees at least one key somewhere
 *                               (safe to skip), 1 = every in-range entry visible, 2 = mixed
 * mask_ndim = 3: mask is [B,L,L];  mask_ndim = 2: mask is [B,L] (the `attn_1d` / retrieval form,
 * cxrbert_origin.py:76-77), broadcast over query rows.  Masked entries contribute the
 * reference's additive -10000.0 (not -inf) inside the kernels.                                 */
int mv_mask_pack(const int64_t* mask, int mask_ndim, int B, int L,
                 uint32_t* bits, uint8_t* tileinfo, void* stream);

/* Same outputs built on the device from per-sample descriptors instead of a materialised [B,L,L] int64 matrix
 * (the reference ships 2 MB / sample at L = 512 from its DataLoader workers, dataset_origin.py:138-176):
 * desc int32 [B,3] = {family, n2, vl}; family 0 full (j < vl), 1 seq2seq, 2 BAR, 3 non-cross, 4 1-D (j < vl);
 * n2 = num_image_embeds + 2; vl = n2 + #text ids incl. [SEP].  Closed forms: SURVEY.md Appendix B.             */
int mv_mask_build(const int32_t* desc, int B, int L, uint32_t* bits, uint8_t* tileinfo, void* stream);

/* ---- on-device mini-batch assembly (MLM corruption, labels, descriptors) ---------------------------
 * Replaces the per-sample python of data/dataset_origin.py:102-135 and CXRDataset.random_word (:183-209).
 * mv_mlm_draws: the two random sources of random_word for every token, from a counter-based hash of `key`:
 *   u   f32   [B,S]  stand-in for random.random(), on a 2^-24 grid in [0,1)
 *   rnd int32 [B,S]  stand-in for random.randrange(vocab)
 *   token (b, t) draws from hash counters 2i and 2i+1, i = b*S + t; B*S <= 2^31-1 (MV_E_SHAPE above)
 * mv_mlm_corrupt consumes draws (these or the caller's own) and raw, un-corrupted ids:
 *   ids     int64 [B,S]   token ids; row b is valid for t < lengths[b] (1 <= lengths[b] <= S; out-of-range is clamped to 0..S, and a
 *                         clamped length of 0 gives [SEP] at t = 0, no label, counts = 0 and n_ids = 1)
 *   family  int32 [B]     attention-mask family per sample for `desc` (see mv_mask_build); NULL = 0 (full)
 * outputs, in the reference's batch protocol (dataset_origin.py:181):
 *   input_txt  int64 [B,T]  T = S+1: corrupted ids, [SEP]=102 at t = lengths[b], [PAD]=0 after
 *   segment    int64 [B,T]  all 1
 *   txt_labels int64 [B,L]  L = S+N+3: -100 except the selected text positions (offset N+2), which carry the original id
 *   n_ids      int32 [B]    lengths[b] + 1
 *   desc       int32 [B,3]  {family, N+2, N+2+n_ids} for mv_mask_build / the attention kernels (nullable)
 *   counts     int32 [B]    labels per sample (scratch the index pass reads)
 *   label_rows / label_ids int32 [>= B*S], n_labels int32 [1] (device): row-major compact index of the labelled
 *                           positions (row = b*L + i) and their ids -- all three NULL to skip.
 * Selection rule per valid token, evaluated in double like the python: u < 0.15 selects; then u/0.15 < 0.8 -> [MASK]=103,
 * < 0.9 -> rnd, else unchanged; a sample with no selection gets token 0 masked and labelled (":204-207").        */
int mv_mlm_draws(unsigned long long key, int B, int S, int vocab, float* u, int32_t* rnd, void* stream);
int mv_mlm_corrupt(const int64_t* ids, const int32_t* lengths, const float* u, const int32_t* rnd, const int32_t* family,
                   int B, int N, int S, int64_t* input_txt, int64_t* segment, int64_t* txt_labels, int32_t* n_ids,
                   int32_t* desc, int32_t* counts, int32_t* label_rows, int32_t* label_ids, int32_t* n_labels, void* stream);

/* HOST function (no device work, no stream): every entry of a materialised reference mask (int64 [B,L,L], or [B,L] for the 1-D
 * family; data/dataset_origin.py:138-176) against the closed form of its descriptor desc[b] = {family, n2, vl} -- the predicates of
 * mv_mask_build, a 32-column word at a time, `threads` host threads split by sample.  *first_mismatch = -1 when every entry agrees,
 * else the linear index (b*L + i)*L + j (b*L + j for 2-D masks) of the first entry that differs.  CXRBERT_Trainer runs it one batch
 * ahead of the step on a worker thread: the descriptors it derives from probe entries are proven bit for bit on EVERY batch without
 * moving the 134 MB matrix over PCIe.  Both pointers are HOST pointers. */
int mv_mask_verify_host(const int64_t* mask, int mask_ndim, const int32_t* desc, int B, int L, int threads, long long* first_mismatch);

/* ---- gradient exchange: RCCL over xGMI (one process per GPU) -----------------------------------------------
 * Replaces nn.DataParallel of models/train_origin.py:53-55 for a host that is not torch (medvill_amd itself reaches the SAME
 * library through torch.distributed's nccl backend, dist.py: a torch process keeps one communicator).  RCCL is loaded at run time
 * (dlopen): MV_E_NO_RCCL when it is absent; a failed RCCL call returns MV_E_COMM_BASE + ncclResult_t.
 *   mv_comm_unique_id        rank 0 makes the 128-byte id, the caller hands it to every rank (any transport)
 *   mv_comm_init             communicator of `world` ranks on the calling thread's current device
 *   mv_comm_allreduce_async  in-place SUM all-reduce of `count` elements (MV_F32 / MV_F16 / MV_BF16), enqueued on `stream`:
 *                            call it per gradient bucket as soon as the backward has finished the bucket, on a side stream
 *   mv_comm_wait             `stream` (the compute stream, before the optimizer) waits -- on the device -- for every collective
 *                            issued so far through this communicator; the host never blocks
 *   mv_comm_destroy                                                                                                    */
int mv_comm_unique_id(void* id128);
int mv_comm_init(void** comm_out, int rank, int world, const void* id128);
int mv_comm_allreduce_async(void* comm, void* buf, size_t count, int dtype, void* stream);
int mv_comm_wait(void* comm, void* stream);
int mv_comm_destroy(void* comm);

/* ---- packed rows (padding removal) -------------------------------------------------------------------
 * In the full, seq2seq and 1-D mask families no valid query can see a position after the sample's text [SEP]
 * (SURVEY.md Appendix B), and those positions carry no label: their rows contribute exactly nothing to the loss,
 * to any gradient or to any valid position's hidden state.  The encoder may therefore run on the valid rows only.
 * mv_pack_plan turns the mask descriptors into the row plan:
 *   cu     int32 [B+1]   exclusive prefix sums of vl[b] = desc[b][2] (clamped to L); cu[B] = number of packed rows
 *   rowmap int32 [>= cu[B]] (capacity B*L)  logical flat position b*L + p of every packed row
 *   inv    int32 [B*L]   packed row of logical position b*L + p, or -1 when it was dropped
 * Consumers: mv_embed_fwd/bwd take (rowmap, n_rows) and read / write packed rows; mv_attn_fwd/bwd take (cu, total_rows)
 * and address qkv / ctx / dctx / dqkv by packed row while mask words, lse, delta and the dropout counter keep their
 * logical [B, L] indexing (so a packed run draws the same attention-dropout masks as the padded one).  All four accept
 * NULL for the dense [B*L] layout.  Packed attention exists for the bf16 MFMA kernels only.                      */
int mv_pack_plan(const int32_t* desc, int B, int L, int32_t* cu, int32_t* rowmap, int32_t* inv, void* stream);
/* Row order of the LAST encoder layer (round 3): attention is equivariant under a reordering of a sample's rows, and in the full / 1-D
 * mask families the mask of a packed sample does not depend on the order either (every row sees every row).  Only the rows the heads
 * consume (`sel`, packed row indices: labelled rows and each sample's first row) are needed as QUERIES of the last layer, so that layer
 * runs on rows reordered with those first and its attention kernels stop after them (qlim of mv_attn_fwd / mv_attn_bwd):
 *   perm    int32 [cu[B]]  packed row (old order) held by row i of the new order
 *   newpos  int32 [cu[B]]  its inverse
 *   qlim    int32 [B]      number of consumed rows of sample b (they are rows cu[b] .. cu[b]+qlim[b]-1 of the new order, ascending old order)
 *   sel_new int32 [n_sel]  newpos[sel[i]] for 0 <= sel[i] < cu[B]; -1 for an entry that lies in no sample (a negative one, such as the
 *                          -1 `inv` holds for a dropped position, or one >= cu[B]): the "no such row" of mv_gather_rows /
 *                          mv_scatter_rows.  The kernel writes every entry; the caller pre-fills nothing.
 * Entries of sel in no sample select nothing; duplicates count once in qlim.  perm / newpos from cu[B] on are not written.
 * L: the logical sequence length (an upper bound of every sample's row count, <= 2048; MV_E_SHAPE above).  */
int mv_tail_perm(const int32_t* cu, int B, int L, const int32_t* sel, int n_sel, int32_t* perm, int32_t* newpos, int32_t* qlim,
                 int32_t* sel_new, void* stream);

/* ---- fused-mask multi-head attention --------------------------------------------------------
 * Replaces HF BertSelfAttention's scores/softmax/context (spec:
 * Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:301-320):
 *   ctx[b,i,h,:] = sum_j softmax_j( q.k/sqrt(dh) + (1-mask)*-10000 ) v
 * qkv is the fused projection output [B*L, 3H] (q | k | v, heads contiguous inside each).
 * lse [B, A, L] (f32) = log-sum-exp of each score row, kept for the backward.
 * dh must be 64 (bf16 MFMA path) or <= 128 (f32 path).
 * p_drop > 0: attention-probability dropout (HF BertSelfAttention.dropout): ctx = dropout(softmax).v; the mask is the
 * tensor of keep-bits `dropbits` written by mv_attn_dropmask (required then), survivors scaled by 1 / (1 - P(drop)) with the
 * P(drop) of that generator: the forward and both backward kernels spend one select per score element (they are bound by vector-instruction
 * issue, not by MFMA, so nothing is hashed inside them).
 * dtype MV_F16: qkv and ctx in the f16 encoding; ctx_bf16 (nullable, MV_F16 only) receives the bf16 copy of ctx that
 * the backward pairs with bf16 gradients.
 * qlim (nullable, int32 [B]): only the first qlim[b] rows of sample b are queries (every row is a key); the context / lse of the other
 * rows are left untouched.  MFMA kernels only.  */
int mv_attn_fwd(int dtype, const void* qkv, const uint32_t* bits, const uint8_t* tileinfo,
                void* ctx, void* ctx_bf16, float* lse, int B, int L, int A, int dh,
                float p_drop, const uint32_t* dropbits, const int32_t* cu, int total_rows, const int32_t* qlim, void* stream);

/* The attention-probability dropout mask of one layer as keep-bits, laid out as the kernels' select masks:
 * dropbits uint32 [B*A][ceil(L/32)][ceil(L/64)][64] (64-byte aligned), i.e. per (head, 32-query block, 64-key tile) 32 x uint64;
 * word 16*kk + r, bit l <-> query 32*qb + (l & 31), key 64*kt + 32*kk + (r&3) + 8*(r>>2) + 4*(l>>5); bit = 1 keeps the entry.
 * Every entry is an independent Bernoulli draw with P(drop) = round(p_drop * 2^n) / 2^n (n = 16: 0.1 -> 0.100006; the debug library has a knob for 12 / 8), a counter-based
 * hash of (drop_key, word index): the same key reproduces the same mask.  Blocks whose queries or keys all lie beyond the
 * sample's packed length (cu, nullable) are not written and never read.  Depends on the key only: it can run ahead of the
 * forward on another stream.  */
int mv_attn_dropmask(float p_drop, unsigned long long drop_key, int B, int L, int A, const int32_t* cu, uint32_t* dropbits,
                     void* stream);

/* dqkv [B*L,3H] from dctx [B*L,H]; `delta` is a [B,A,L] f32 scratch (rowsum(dctx*ctx)).  dtype (MV_F32, MV_BF16 or
 * MV_F16) is the encoding of qkv, ctx, dctx and dqkv alike.  qlim (nullable): as in mv_attn_fwd; the dctx rows past a sample's
 * limit are ignored (taken as zero) and their dQ rows are written as zeros.
 * Alignment (16-bit MFMA path; MV_E_SHAPE otherwise): qkv and dctx 16 bytes, dqkv 8 bytes (mv_attn_fwd: qkv 16, ctx and ctx_bf16 8,
 * dropbits 64).  ctx is not checked here: the kernels read it through a buffer descriptor in 16-byte pieces at element offsets that
 * are multiples of 8, which needs the element alignment of the encoding only. */
int mv_attn_bwd(int dtype, const void* qkv, const void* ctx, const void* dctx, const float* lse,
                const uint32_t* bits, const uint8_t* tileinfo,
                void* dqkv, float* delta, int B, int L, int A, int dh,
                float p_drop, const uint32_t* dropbits, const int32_t* cu, int total_rows, const int32_t* qlim, void* stream);

/* The attention probabilities of one layer, from what its forward left behind (qkv, lse, mask words, tile classes, keep-bits):
 *   P[b,a,i,j] = exp(q_i.k_j / sqrt(dh) + (mask[b,i,j] ? 0 : -10000) - lse[b,a,i])
 * -- HF BertSelfAttention's attention_probs (model.py:301-320 with output_attentions), the third value of the encoder protocol
 * (models/cxrbert_origin.py:126-130).  Dense [B*L] row layout only (no packed rows, no query limit).
 *   dtype      encoding of qkv (MV_F32, MV_BF16, MV_F16); out_dtype: MV_F32 or that same encoding (anything else: MV_E_ARG)
 *   probs      [B, A, L, L] row-major, or [B, L, L] when head_mean != 0: the arithmetic mean over the A heads, summed in f32 by the
 *              one thread block that owns the tile (no atomics, no second pass).  Nothing outside it is written.
 *   p_drop > 0 the keep-bits `dropbits` of mv_attn_dropmask are applied and survivors scaled as in mv_attn_fwd: the result is the
 *              matrix the context was computed from (what HF returns in train mode).
 * Tiles of class 0 (skipped by the forward) are written as zeros: every one of their entries is exp(-10000 + ...) = 0 in fp32.
 * 16-bit path: dh must be 64 (v_mfma_f32_32x32x16_{f16,bf16}; 16-byte stores when L is a multiple of 4 (f32 output) / 8 (16-bit
 * output), element stores otherwise); f32 path and the debug library's impl knob: dh <= 128.  ceil(L/64) <= 64.
 * MV_E_ARG: a null pointer, a size that is not positive, a bad out_dtype, p_drop > 0 without dropbits.  MV_E_SHAPE: the limits above,
 * qkv or probs not 16-byte aligned, dropbits not 64-byte aligned, a qkv of 2^31 bytes or more on the 16-bit path (it is read through a
 * buffer descriptor; probs is addressed with 64-bit offsets and has no such limit).  A refused call launches nothing. */
int mv_attn_probs(int dtype, const void* qkv, const uint32_t* bits, const uint8_t* tileinfo, const float* lse, void* probs,
                  int out_dtype, int B, int L, int A, int dh, float p_drop, const uint32_t* dropbits, int head_mean, void* stream);

/* ---- LayerNorm ------------------------------------------------------------------------------
 * y = (x-mean)/sqrt(var+eps)*gamma+beta over the last dim (HF LayerNorm eps=1e-12 in the
 * encoder; TF-style BertLayerNorm eps=1e-5 of cxrbert_origin.py:189-202 in the MLM head).
 * x_dtype: dtype of x (the fused-residual GEMM writes f32); y in `dtype`; y_bf16 (nullable, dtype MV_F16 only): bf16
 * copy of y for the backward's weight-gradient product.  mean, rstd: f32 [M], kept for backward.  */
int mv_layernorm_fwd(int dtype, const void* x, int x_dtype, const float* gamma, const float* beta,
                     void* y, void* y_bf16, float* mean, float* rstd, int M, int H, float eps, void* stream);

/* dx (dtype) = LN backward of dy (dtype) w.r.t. x; dgamma/dbeta (f32 [H]) are ACCUMULATED
 * (atomically) -- zero them first; colsum (f32 [H], nullable) accumulates sum_m dx[m,:]
 * (the bias gradient of the projection that produced x).
 * dx_drop (nullable): second output = dx * dropout_mask / (1 - p), the gradient w.r.t. the projection
 * output when x = dropout(projection) + residual (mask index m*H + c); colsum then sums dx_drop.
 * grad_unscale_dev (nullable): *grad_unscale_dev multiplies what is added to dgamma / dbeta / colsum (1 / loss scale). */
int mv_layernorm_bwd(int dtype, const void* dy, const void* x, int x_dtype, const float* mean,
                     const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta,
                     float* colsum, int M, int H,
                     void* dx_drop, float p_drop, unsigned long long drop_key, const float* grad_unscale_dev, void* stream);

/* ---- sequence assembly + embeddings ---------------------------------------------------------
 * Replaces CXRBertEncoder.forward's else-branch assembly (cxrbert_origin.py:114-125),
 * ImageBertEmbeddings.forward (:22-35) and the four HF BertEmbeddings calls: writes
 *   x0[b] = LN( [ E[cls]+Ty[0]+P[0] | imgproj[b,n]+P[img_pos[b,n]]+Ty[0] | E[sep]+Ty[0]+P[0] |
 *               E[txt[b,t]]+Ty[segment[b,t]]+P[t] ] )         L = N + T + 2
 * straight into the concatenated [B,L,H] buffer.  imgproj = feats.Wi^T + bi comes from mv_gemm.
 * Tables E, P, Ty and imgproj are in `dtype`; gamma/beta f32.  `pre` (f32 [B,L,H]) keeps the
 * pre-LayerNorm sums for the backward.  x0_bf16 (nullable, dtype MV_F16 only): bf16 copy of x0.
 * img_pos NULL: the image rows get NO position embedding (args.img_postion false, cxrbert_origin.py:27-31).
 * p_drop: dropout of the text / [CLS] / [SEP] rows (HF hidden_dropout_prob); p_drop_img: of the image rows
 * (ImageBertEmbeddings' nn.Dropout(args.dropout_prob), cxrbert_origin.py:19); same key and element index.  */
int mv_embed_fwd(int dtype, const int64_t* cls_tok, const int64_t* txt, const int64_t* segment,
                 const int64_t* img_pos, const int64_t* sep_tok, const void* imgproj,
                 const void* E, const void* P, const void* Ty, const float* gamma, const float* beta,
                 void* x0, void* x0_bf16, float* pre, float* mean, float* rstd,
                 int B, int N, int T, int H, int V, int maxpos, float eps,
                 float p_drop, float p_drop_img, unsigned long long drop_key, const int32_t* rowmap, int n_rows, void* stream);

/* Backward of the above: LN backward of dx0, scatter-add (f32 atomics) into dE [V,H], dP, dTy,
 * dgamma, dbeta (all ACCUMULATED) and write d(imgproj) [B,N,H] in `dtype`.  Row `pad_token_id`
 * of dE receives no look-up gradient (HF BertEmbeddings builds nn.Embedding(..., padding_idx=
 * pad_token_id = 0)); pass -1 for none.  grad_unscale_dev (nullable): factor on everything added to the f32 gradients. */
int mv_embed_bwd(int dtype, const void* dx0, const float* pre, const float* mean, const float* rstd,
                 const float* gamma, const int64_t* cls_tok, const int64_t* txt, const int64_t* segment,
                 const int64_t* img_pos, const int64_t* sep_tok,
                 float* dE, float* dP, float* dTy, float* dgamma, float* dbeta, void* dimgproj,
                 int B, int N, int T, int H, int V, int maxpos, int pad_token_id,
                 float p_drop, float p_drop_img, unsigned long long drop_key, const int32_t* rowmap, int n_rows,
                 const float* grad_unscale_dev, void* stream);

/* ---- losses + step metrics ------------------------------------------------------------------
 * Replaces nn.CrossEntropyLoss(ignore_index=-100) on mlm.transpose(1,2) and
 * nn.CrossEntropyLoss() on the ITM logits (train_origin.py:62-63,120-126) plus the argmax
 * metrics of train_origin.py:133-146, fused with the loss gradient.
 * logits [R, ld] (l_dtype f32, bf16 or f16); labels int32 [R] (-100 = ignored row);
 * any label outside 0..V-1 (negative, or >= V where torch would raise) is an ignored row: no loss,
 * no count, a zero gradient row; the logits of such a row are not read.
 * out[0] += sum of nll over labelled rows, out[1] += #labelled rows, out[2] += #rows whose
 * argmax == label (f32 accumulators, zero them first).
 * dlogits (nullable; d_dtype) = (softmax - onehot) * grad_scale for labelled rows, 0 otherwise;
 * columns V..ldd-1 are zero-filled (so dlogits can feed mv_gemm with K = V).
 * grad_scale is read from the device (*grad_scale_dev) when non-null (so 1/n_labelled_global
 * can be produced by an all-reduce without a host sync), else grad_scale_host; loss_scale_dev
 * (nullable) multiplies it by the loss scale of the f16-gradient path (device state [0]).       */
int mv_ce_fwd_bwd(const void* logits, int l_dtype, int ld, const int32_t* labels, int R, int V,
                  float* out, void* dlogits, int d_dtype, int ldd,
                  const float* grad_scale_dev, float grad_scale_host, const float* loss_scale_dev, void* stream);

/* ---- row gather / scatter (labelled-row compaction for the MLM head) ------------------------
 * dst[i,:] = src[rows[i],:]  /  dst[rows[i],:] (+)= src[i,:]; rows int32 [R].  A negative rows[i] means "no such
 * row" (a position dropped by mv_pack_plan): gather writes zeros, scatter writes nothing.
 * scatter: the non-negative rows[i] must be distinct -- two source rows with the same destination race (with or without
 * accumulate) and the result is unspecified.  accumulate adds in f32 and rounds once to dtype.          */
int mv_gather_rows(int dtype, const void* src, int lds, const int32_t* rows, int R, int H,
                   void* dst, int ldd, void* stream);
int mv_scatter_rows(int dtype, const void* src, int lds, const int32_t* rows, int R, int H,
                    void* dst, int ldd, int accumulate, void* stream);

/* out[n] (+)= [*grad_unscale_dev] * sum_m x[m,n]  (bias gradients). x [M,N] in dtype, out f32.   */
int mv_colsum(int dtype, const void* x, int ldx, int M, int N, float* out, int accumulate, const float* grad_unscale_dev,
              void* stream);
/* out[n] += [*grad_unscale_dev] * sum_{p < P} part[p*ld + n]: folds the partial column sums written by mv_gemm (colsum_part). */
int mv_colsum_partials(const float* part, int P, int ld, int N, float* out, const float* grad_unscale_dev, void* stream);

/* elementwise c = a + b (dtype), n elements */
int mv_add(int dtype, const void* a, const void* b, void* c, size_t n, void* stream);

/* out = dy * gelu_erf'(z) (mode 0; backward of the MLM transform's activation,
 * cxrbert_origin.py:176-181,216), out = dy * (1 - z*z) (mode 1; tanh backward of the pooler,
 * z holds the tanh OUTPUT) or out = dy * (z > 0) (mode 2; ReLU backward of the VQA answer classifier, z holds the ReLU
 * OUTPUT).  n elements, n % 4 == 0. */
int mv_dact(int dtype, int mode, const void* dy, const void* z, void* out, size_t n, void* stream);

/* 2-D cast: dst[r, 0..cols) = src[r, 0..cols), dst[r, cols..ldd) = 0 (pads a [rows, V] gradient
 * to a leading dimension the MFMA GEMM accepts). */
int mv_cast2d(const void* src, int src_dtype, long long lds, void* dst, int dst_dtype, long long ldd,
              int rows, int cols, void* stream);

/* dst[c, r] = src[r, c] for r < rows, c < cols (leading dimensions lds >= cols, ldd >= rows; same dtype both sides).
 * Utility (the training engine keeps one transposed copy per layer: the FFN-down weights, for dz as an NT-form GEMM). */
int mv_transpose(int dtype, const void* src, long long lds, void* dst, long long ldd, int rows, int cols, void* stream);

/* dst(dst_dtype) = src(src_dtype), n elements */
int mv_cast(const void* src, int src_dtype, void* dst, int dst_dtype, size_t n, void* stream);

/* ---- region-feature extractor: ResNet-50 trunk pieces (models/image.py:46-69) ------------------------------
 * The trunk runs in NHWC: an activation is the matrix [B*H*W, C] and every convolution is mv_gemm over it -- directly
 * for 1x1 / stride 1, after mv_im2col otherwise (weights re-laid as [Cout, kh*kw*Cin], (ky, kx, c) order).  BatchNorm
 * (+ residual)(+ ReLU) is mv_bn_act, with batch statistics from mv_col_stats in train() mode or the running ones in
 * eval().  Forward only: the reference never trains the CNN (cxrbert_origin.py:66-70 unfreezes nothing).
 *   mv_nchw_to_nhwc : f32 [B,C,H,W] -> dst_dtype [B,H,W,Cp], channels C..Cp-1 zero
 *   mv_im2col       : src [B,H,W,C] -> dst [B*Ho*Wo, ldk], column (ky*kw + kx)*C + c = src[b, oy*stride-pad+ky, ox*stride-pad+kx, c]
 *                     (0 outside the image; columns kh*kw*C..ldk-1 zero), Ho = (H + 2*pad - kh)/stride + 1
 *   mv_col_stats    : stats f32 [2, C] = per-column sum and sum of squares over the rows of x [rows, C] (C, ldx % 4 == 0)
 *   mv_bn_finalize  : mean / rstd of the batch from those sums (biased variance), plus nn.BatchNorm2d's momentum update of
 *                     running_mean / running_var (unbiased variance) when they are given (both or neither)
 *   mv_bn_act       : y = (x - mean) * rstd * gamma + beta (+ residual) (max 0 when relu != 0); C % 4 == 0; x may be f32
 *                     while y / residual are bf16
 *   mv_maxpool3x3s2 : 3x3 / stride 2 / pad 1 max pooling, NHWC; C % 4 == 0
 * Alignment: mv_col_stats, mv_bn_act and mv_maxpool3x3s2 move four elements per access, so x, y and residual must be aligned to
 * four of their elements (8 bytes of bf16, 16 of f32) and mean / rstd / gamma / beta to 16 bytes: MV_E_SHAPE otherwise.
 * mv_im2col takes any element-aligned base (it gathers element by element unless both bases are 16-byte aligned), and so does
 * mv_nchw_to_nhwc.  Null pointers and non-positive sizes, Cp < C: MV_E_ARG; ldk < kh*kw*C, an output size that is not positive,
 * C or ldx not a multiple of 4: MV_E_SHAPE; MV_F16, or f32 y from bf16 x: MV_E_DTYPE.  A refused call writes nothing.      */
int mv_nchw_to_nhwc(const float* src, void* dst, int dst_dtype, int B, int C, int H, int W, int Cp, void* stream);
int mv_im2col(int dtype, const void* src, int B, int H, int W, int C, int kh, int kw, int stride, int pad, void* dst, int ldk,
              void* stream);
/* y[(b,oy,ox), o] = sum_{ky,kx,c} x[b, oy*stride-pad+ky, ox*stride-pad+kx, c] * w[o, (ky*kw + kx)*C + c]  (NHWC x, zero padding):
 * the convolution as an implicit GEMM on the MFMA kernel -- the activation operand is gathered tap by tap while it is
 * staged, no patch matrix is materialised.  bf16 x / w, y in y_dtype; C a power of two >= 8, O % 4 == 0.
 * epi: MV_EPI_NONE, MV_EPI_BIAS, MV_EPI_BIAS_RELU or MV_EPI_BIAS_RES_RELU (R [rows, O], leading dimension O).          */
int mv_conv2d(int dtype, const void* x, const void* w, void* y, int y_dtype, int B, int H, int W, int C, int O, int kh, int kw,
              int stride, int pad, const float* bias, int epi, const void* R, int r_dtype, void* stream);
int mv_col_stats(int dtype, const void* x, int ldx, int rows, int C, float* stats, void* stream);
int mv_bn_finalize(const float* stats, int C, long long rows, float eps, float momentum, float* mean, float* rstd,
                   float* running_mean, float* running_var, void* stream);
int mv_bn_act(int dtype, const void* x, int x_dtype, const float* mean, const float* rstd, const float* gamma, const float* beta,
              const void* residual, void* y, long long rows, int C, int relu, void* stream);
int mv_maxpool3x3s2(int dtype, const void* x, void* y, int B, int H, int W, int C, void* stream);

/* ---- dropout mask (inspection / tests) -----------------------------------------------------------
 * The kernels above never store dropout masks: they regenerate them from a counter-based hash of
 * (drop_key, linear element index).  keep[i] = 1 if element i survives; an element is dropped with
 * probability round(p_drop*65536)/65536 and survivors are scaled by *scale_out (HOST pointer, nullable).
 * These are the masks of the hidden-state sites (embeddings, both projections); the attention-probability site's mask is
 * the keep-bit tensor of mv_attn_dropmask. */
int mv_dropout_mask(float p_drop, unsigned long long drop_key, size_t n, uint8_t* keep, float* scale_out,
                    void* stream);

/* ---- optimizer ------------------------------------------------------------------------------
 * HF transformers.optimization.AdamW (<= 4.x) as called at train_origin.py:60,131:
 *   m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g*g; p -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps);
 *   p -= lr*wd*p            (eps added BEFORE the bias correction, decoupled decay)
 * over one flat f32 buffer of n elements (all parameters live in one flat buffer);
 * g is multiplied by grad_scale first; shadow_bf16 / shadow_f16 (nullable) receive the 16-bit copies of
 * the updated parameters that the MFMA kernels read.
 * scaler_state (nullable; the f32 [8] device state of mv_scaler_update): when given, the step is SKIPPED entirely if
 * state[3] != 0 (the backward overflowed) and t of the bias correction is state[4] instead of `step`.   */
int mv_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, void* shadow_f16, size_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  int correct_bias, float grad_scale, const float* scaler_state, void* stream);

/* ---- dynamic loss scale of the f16-gradient path -------------------------------------------
 * No counterpart in the reference (its gradients never leave f32; train_origin.py:129-131): f16 gradient operands need
 * the loss scaled into f16's range.  state f32 [8] on the device: [0] scale S (read by mv_ce_fwd_bwd as loss_scale_dev),
 * [1] 1/S (read as grad_unscale_dev / alpha_dev), [2] clean steps since S changed, [3] skip flag, [4] optimizer steps
 * applied, [5] steps skipped, [6] non-finite count.  Initialise to {S0, 1/S0, 0, 0, 0, 0, 0, 0}.
 *   mv_count_nonfinite: counter[0] += #elements of x (f32 [n], 16-byte aligned) that are inf or nan
 *   mv_scaler_update  : count > 0 -> skip = 1, S = max(S*backoff, min_scale); else skip = 0, t += 1 and after
 *                       growth_interval clean steps S = min(S*growth, max_scale); clears the count.        */
int mv_count_nonfinite(const float* x, size_t n, float* counter, void* stream);
int mv_scaler_update(float* state, int growth_interval, float growth, float backoff, float max_scale, float min_scale,
                     void* stream);

/* ---- report generation (KV-cached decode, csrc/mv_decode.hip) -------------------------------------
 * Replaces the incremental decoder of the reference's report-generation code
 * (Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:1132-1487, driven by generation_decode.py),
 * which re-projects the whole history at every step.  Here every layer keeps a cache of K / V rows ("slots"); each new query
 * row lists the slots it sees.  Additive entry points: the pretraining path does not call them.
 *
 * mv_gemm_rows: C[M,N] = epi(x[M,K] . W[N,K]^T) for a few rows (M <= 256): the weights are streamed once, 16-bit operands
 *   (dtype MV_BF16 / MV_F16), f32 accumulation.  epi: MV_EPI_NONE, MV_EPI_BIAS, MV_EPI_BIAS_GELU (C = gelu_erf(x.W^T + bias);
 *   no pre-activation output), MV_EPI_BIAS_RELU (C = max(x.W^T + bias, 0); the VQA answer classifier) or MV_EPI_BIAS_RES
 *   (C = x.W^T + bias + R, R in r_dtype); C in c_dtype (f32 for the LayerNorm
 *   that follows a residual sum, and for logits).  K % 32 == 0, ldx / ldw multiples of 8, 16-byte aligned x and W.
 *   Separate from mv_gemm, whose routing is unchanged.
 * mv_attn_decode: for query row r (q [R, ldq], heads of dh contiguous) and head h:
 *     ctx[r, h] = sum_j softmax_j( q[r,h] . K[s_j, h] / sqrt(dh) ) V[s_j, h],   s_j = slots[row(r)][j], j < nk[r]
 *   row(r) = slot_row[r] (int32, nullable: r) -- beams of one sample share a table row prefix, and the MASK row and the token row
 *   of one beam share one table row with different nk.  K / V caches: [slots, ldkv] in dtype (f32, bf16, f16), f32 softmax.
 *   max_nk >= every nk[r] (host bound; picks the split count).  dh <= 128, 256 % dh == 0.  nk[r] = 0 yields a zero context row.
 *   nsplit: 1 = one pass; > 1 = split-KV: the key list is cut in nsplit ranges whose (context, max, sum) partials go to ws
 *   (>= nsplit * R * A * (dh + 2) floats) and are merged through the log-sum-exp; 0 = the library picks (as many as ws holds).
 * mv_logprob_topk: per row of logits [R, ld] (f32): lse = log sum exp, logp = x - lse; eos_penalty_id >= 0 sets logp of that
 *   column to -10000.0 (after the normalisation, as the reference's min_len rule); vals f32 [R,k] / idx int64 [R,k] = the k
 *   largest logp (k <= 16) in descending order, ties to the lower column.  lse (nullable) f32 [R].  No [R,V] output.
 *   A -inf logit adds nothing to lse and ranks last (logp -inf, by column); a row that is -inf throughout is outside the contract.
 * mv_embed_rows: out[r] = LN(E[ids[r]] + Ty[seg[r]] + P[pos[r]]) (HF BertEmbeddings of one token), tables in dtype, gamma /
 *   beta f32; indices int64, clamped into their tables.  The tables are dense: row i of E / P / Ty starts at element i * H.
 *
 * n-gram blocking (the reference decoder's forbid_duplicate_ngrams / ngram_size / forbid_ignore_set, model.py:1373-1426, kept on
 * the device).  Two additive entry points:
 * mv_ngram_ban: one beam step for R beams whose histories hold `len` words each.
 *     hist_out[r, :len] = hist_in[parent[r], :len],  hist_out[r, len] = (int32)y[r]
 *   hist_in / hist_out int32 [R, ld_h]; parent int64 [R] (what torch index arithmetic on the back pointers gives; nullable:
 *   identity; a value outside [0, R) reads row 0 / R-1); y int64 [R].  hist_out must not overlap hist_in (MV_E_ARG): the gather
 *   reads rows other blocks write.  With seq = hist_out[r, :len+1] and tail = its last n-1 words, the banned words of beam r are
 *     none when len + 1 < n, none when a word of tail is in ignore, else every seq[i+n-1] with seq[i:i+n-1] == tail
 *     (0 <= i <= len+1-n; the last windows overlap the tail, so a run of one word bans that word) that is not in ignore;
 *   ban int32 [R, ld_ban] receives them once each in ascending order, nban int32 [R] their number.  Columns of ban at and
 *   beyond nban[r] and columns of hist_out beyond len are not written.  ignore int32 [n_ign], nullable when n_ign = 0.
 *   Limits: 2 <= n <= 8 (MV_E_ARG); len + 1 <= ld_h, len + 1 <= 1024, n_ign <= 256, ld_ban >= len + 2 - n (MV_E_SHAPE).
 * mv_logprob_topk_banned: mv_logprob_topk on  logp[c] = fl(x[c] - lse),  logp[c] = fl(logp[c] - 10000) for every c listed in
 *   ban[r, :nban[r]] (int32 [R, ld_ban] / int32 [R]; ids outside [0, V) are ignored, an id listed twice counts once), then
 *   logp[eos_penalty_id] = -10000 exactly (also when that column is banned).  Banned columns stay in lse.  A banned column
 *   ranks by its penalised value, ties to the lower column.  ban == NULL, or nban[r] == 0, gives the bits mv_logprob_topk
 *   gives (vals, idx, lse).  V <= 131072 (one LDS bit per column; MV_E_SHAPE), k <= 16, k <= V.  nban[r] is clamped to
 *   [0, ld_ban].  Rows whose unbanned log-probs themselves reach -10000 are outside the contract.  */
int mv_gemm_rows(int dtype, int M, int N, int K, const void* x, int ldx, const void* W, int ldw, void* C, int ldc, int c_dtype,
                 const float* bias, int epi, const void* R, int ldr, int r_dtype, void* stream);
int mv_attn_decode(int dtype, const void* q, int ldq, const void* k_cache, const void* v_cache, int ldkv, const int32_t* slots,
                   int ld_slots, const int32_t* slot_row, const int32_t* nk, int max_nk, void* ctx, int ldo, int R, int A, int dh,
                   int nsplit, float* ws, size_t ws_bytes, void* stream);
int mv_logprob_topk(const float* logits, int ld, int R, int V, int k, int eos_penalty_id, float* vals, int64_t* idx, float* lse,
                    void* stream);
int mv_embed_rows(int dtype, const int64_t* ids, const int64_t* pos, const int64_t* seg, const void* E, const void* P, const void* Ty,
                  const float* gamma, const float* beta, void* out, int ldo, int R, int H, int V, int maxpos, int ntype, float eps,
                  void* stream);
int mv_ngram_ban(const int32_t* hist_in, int32_t* hist_out, int ld_h, const int64_t* parent, const int64_t* y, int R, int len, int n,
                 const int32_t* ignore, int n_ign, int32_t* ban, int ld_ban, int32_t* nban, void* stream);
int mv_logprob_topk_banned(const float* logits, int ld, int R, int V, int k, int eos_penalty_id, const int32_t* ban, int ld_ban,
                           const int32_t* nban, float* vals, int64_t* idx, float* lse, void* stream);

/* ---- VQA fine-tuning and answer prediction (csrc/mv_vqa.hip) --------------------------------------
 * The answer classifier of the reference's VQA model (Downstream_task/report_generation_and_vqa/sc/pytorch_pretrained_bert/
 * model.py:939-943,979-983,1016-1041): Linear(H, 2H) + ReLU + Linear(2H, A), nn.BCEWithLogitsLoss over soft targets, the
 * argmax score split by answer type.  The two products run on mv_gemm_rows / mv_gemm.  Additive entry points.
 *
 * mv_bce_fwd_bwd: per row r of logits [R, ld] (f32) and soft targets [R, A] (f32, contiguous; nullable when stats and dgrad are):
 *     stats[1] += sum_c max(z,0) - z*y + log1p(exp(-|z|))                                      (the loss SUM; mean = / (R*A))
 *     dgrad[r, c] = (sigmoid(z) - y) * g * S  for c < A, 0 for A <= c < ldd   (d_dtype; g = *grad_scale_dev when non-null, else
 *                   grad_scale_host; S = *loss_scale_dev when non-null, else 1 -- as mv_ce_fwd_bwd)
 *     arg_train[r] = argmax_c z (int64), arg_infer[r] = argmax_{c >= 1} z (int64, the column itself: the "+1" is included);
 *                   ties to the lower column
 *     stats f32 [6] += {y[arg_train], loss, closed score, closed count, open score, open count}: ans_type int32 [R] (nullable)
 *                   0 = CLOSED, 1 = OPEN; any other value counts in neither split (zero stats first).
 *   stats, dgrad, arg_train and arg_infer are each nullable (inference needs neither loss nor gradient).
 * mv_rows_mul: out[i, :H] = a[rows_a[i], :H] * b[rows_b[i], :H] (dtype; a negative row index gives zeros).  H and the leading
 *   dimensions multiples of 4, bases aligned to 4 elements.                                                                    */
int mv_bce_fwd_bwd(const float* logits, int ld, const float* target, const int32_t* ans_type, int R, int A, float* stats,
                   void* dgrad, int d_dtype, int ldd, const float* grad_scale_dev, float grad_scale_host, const float* loss_scale_dev,
                   int64_t* arg_train, int64_t* arg_infer, void* stream);
int mv_rows_mul(int dtype, const void* a, int lda, const int32_t* rows_a, const void* b, int ldb, const int32_t* rows_b, int R, int H,
                void* out, int ldo, void* stream);

/* ---- BertAdam and multi-label classification (csrc/mv_optim.hip) ------------------------------------
 * The optimizer of every fine-tuning program of the reference (pytorch_pretrained_bert/optimization.py:57-182).  Additive entry points.
 *
 * Both optimizer calls read two device tables over a flat f32 buffer of n elements (n % 4 == 0, 16-byte aligned):
 *   tensors int64 [T, 4] = {offset, count, first_chunk, flags}; offset % 64 == 0; flags bit 0: weight decay applies, bit 1: active
 *   chunks  int32 [NC]   = tensor id per chunk of MV_OPTIM_CHUNK elements; tensor t owns chunks first_chunk ..
 *                          first_chunk + ceil(count / MV_OPTIM_CHUNK) - 1, in element order
 * mv_tensor_sqnorms: out[t] = sum of x[offset .. offset + count)^2 for every active tensor (0 for an inactive one); partials is an
 *   f32 [NC] workspace.  Fixed summation order, no atomics: the same input gives the same bits on every run.
 * mv_bertadam_step: for every element of every active tensor
 *     g' = g * min(1, max_grad_norm / (sqrt(sqnorms[t]) + 1e-6))        (max_grad_norm > 0; sqnorms from mv_tensor_sqnorms)
 *     m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2  (1 - b formed in double, rounded once);  u = m / (sqrt(v) + eps) [+ weight_decay * p when flagged]
 *     p -= lr_t u,  lr_t = lr * schedule(step / t_total, warmup) (t_total == -1: lr), no bias correction; `step` is the number of
 *     updates applied BEFORE this one.  shadow_bf16 / shadow_f16 (nullable) receive the updated p.  g is not modified.  Elements
 *     outside every tensor and inactive tensors are neither read nor written.
 *   scaler_state (nullable, as mv_adamw_step): state[3] != 0 skips the whole step; otherwise step = max(state[4] - 1, 0) (mv_scaler_update
 *     has already counted the step being applied), so a skipped step does not advance the schedule.
 * mv_bce_multilabel (the loss of the diagnosis classifier, Downstream_task/Classification/mmbt/main.py:93-101): per row of logits
 *   [R, ld] (f32), multi-hot targets [R, C] (f32, contiguous) and pos_weight w [C] (nullable = 1):
 *     *loss += sum_c (1 - y) z + (1 + (w - 1) y) (max(-z, 0) + log1p(exp(-|z|)))                  (the SUM; mean = / (R*C))
 *     dgrad[r, c] = (sigmoid(z) (w y + 1 - y) - w y) * g * S for c < C, 0 for C <= c < ldd         (g, S as mv_bce_fwd_bwd)
 *     probs[r, c] = sigmoid(z)  (f32 [R, C]);  counters f32 [3, C] += {tp, fp, fn} with prediction z > 0 and label y > 0.5
 *   target, pos_weight, loss, dgrad, probs and counters are each nullable (loss, dgrad and counters need target).                */
#define MV_OPTIM_CHUNK 4096
enum { MV_SCHED_WARMUP_LINEAR = 0, MV_SCHED_WARMUP_CONSTANT = 1, MV_SCHED_WARMUP_COSINE = 2 };
int mv_tensor_sqnorms(const float* x, size_t n, const int64_t* tensors, int T, const int32_t* chunks, int NC, float* partials,
                      float* out, void* stream);
int mv_bertadam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, void* shadow_f16, size_t n,
                     const int64_t* tensors, int T, const int32_t* chunks, int NC, const float* sqnorms, double lr, double b1, double b2,
                     float eps, float weight_decay, float max_grad_norm, int step, int t_total, double warmup, int schedule,
                     const float* scaler_state, void* stream);
int mv_bce_multilabel(const float* logits, int ld, const float* target, const float* pos_weight, int R, int C, float* loss,
                      void* dgrad, int d_dtype, int ldd, const float* grad_scale_dev, float grad_scale_host,
                      const float* loss_scale_dev, float* probs, float* counters, void* stream);

/* ---- Report-generation fine-tuning (csrc/mv_lmloss.hip) ----------------------------------------------
 * The masked-LM objective of the reference's BertForPreTrainingLossMask(tasks='report_generation') (Downstream_task/
 * report_generation_and_vqa/sc/pytorch_pretrained_bert/model.py:998-1005,1043-1054, loss.py:12-48).  Additive entry points.
 *
 * logits f32 [U, ld] (ld >= V): one row per DISTINCT consumed position.  The prediction entries are stored in CSR form over those
 * rows: row u owns entries row_ptr[u] .. row_ptr[u+1]-1 (row_ptr int32 [U+1], row_ptr[U] = n_entries); entry e has labels[e] (int32,
 * 0 <= label < V), weights[e] (f32 >= 0) and sample[e] (int32, 0 <= sample < B).  Several entries may share a row, with equal or
 * different labels.  label_smoothing in [0, 1]; with smoothing V >= 3, c = 1 - label_smoothing, s = f32(label_smoothing / (V-2)).
 * mv_lm_loss_fwd: per row one pass (max, sum of exponentials, sum of the logits over columns 1..V-1, first argmax); per entry
 *     entry_loss[e] = lse - z[label]                                                       (label_smoothing == 0; label 0 counts)
 *                   = 0                                                                    (smoothing, label 0: ignored)
 *                   = c log c + (V-2) s log s - c (z[t] - lse) - s ((zsum - z[t]) - (V-2) lse)     (smoothing; 0 log 0 = 0)
 *     entry_hit[e] (int32, nullable) = argmax == label;  row_stat f32 [U, 2] = {max, sum exp(z - max)} for the backward.
 * mv_lm_loss_select (one launch of one block, B <= 2048): per-sample sums of w * loss and of w in entry order (double, no atomics:
 *     bitwise reproducible); keep[b] (int32 [B]) = 1 for the k samples with the smallest loss sums, ties to the lower sample index;
 *     stats f32 [4] = {sum of kept loss sums / (kept weight sum + 1e-5), kept weight sum, kept sample count, entries of kept samples
 *     with weight > 0 whose argmax equals the label}; *inv_denom = 1 / (kept weight sum + 1e-5).  k = 0: loss 0, nothing kept.
 * mv_lm_loss_bwd: dlogits[u, c] = g S inv_denom sum over the row's entries with keep[sample] != 0 of w (Q softmax[c] - q[c]) for c < V
 *     and 0 for V <= c < ldd (d_dtype f32 / bf16 / f16); q = the entry's target row (one-hot without smoothing; with it 0 in column 0,
 *     c at the label, s elsewhere, and all zero for label 0), Q = its sum; g = *grad_dev, S = *loss_scale_dev (nullable = 1).  A row
 *     without a kept entry of positive weight and mass is written as zeros and its logits are not read.
 * U = 0 launches nothing.  Null pointers, negative counts, ld < V, V < 3 under smoothing: MV_E_ARG; ldd < V, B > 2048: MV_E_SHAPE.  */
int mv_lm_loss_fwd(const float* logits, int ld, int U, int V, const int32_t* row_ptr, const int32_t* labels, int n_entries,
                   double label_smoothing, float* entry_loss, int32_t* entry_hit, float* row_stat, void* stream);
int mv_lm_loss_select(const float* entry_loss, const float* weights, const int32_t* sample, const int32_t* entry_hit, int n_entries,
                      int B, int k, int32_t* keep, float* stats, float* inv_denom, void* stream);
int mv_lm_loss_bwd(const float* logits, int ld, int U, int V, const int32_t* row_ptr, const int32_t* labels, const float* weights,
                   const int32_t* sample, int n_entries, double label_smoothing, const float* row_stat, const int32_t* keep,
                   const float* inv_denom, const float* grad_dev, const float* loss_scale_dev, void* dlogits, int d_dtype, int ldd,
                   void* stream);

/* ---- image-report retrieval from device-resident banks (csrc/mv_retrieval.hip) ---------------------------------------------
 * The reference's Downstream_task/Retrieval/full_dset_retrieval.py: the training sampler of CXR_Retrieval_Dataset.__getitem__
 * (:108-143), the pair batches of data_processing (:172-215) and the ranking metrics of compute_ranks / compute_recall_precision /
 * compute_mrr (:250-324).  Additive entry points.
 *
 * mv_pair_draws: the sampler's random words.  draws uint32 [B, D, 2] (D <= 300): entry (i, t) = the two words {w0, w1} of attempt t
 *     of sample i, from the counter-based hash keyed by (key, step) at counters 2c, 2c + 1 with c = 300 i + t.
 * mv_pair_negatives: for positive i with dataset index d = idx[i] (int32 [B], clamped to [0, n)) in a dataset of n >= 2 items:
 *     r = (uint64(w0) * (n - 1)) >> 32, other = r + (r >= d); the negative is (image other, text d) when w1's top bit is set, else
 *     (image d, text other).  class_id int32 [n] (nullable; the reference's label_conditioned mode): attempts t = 0, 1, ... are drawn
 *     while class_id[other] == class_id[d], at most 300, and the last one is kept.  draws (nullable) uint32 [B, n_draws, 2] replaces
 *     the hash (attempt t reads entry t; at most min(n_draws, 300) attempts), else the words are those of mv_pair_draws.
 *     pairs int32 [2B, 2] = (image item, text item): the B positives (d, d), then the B negatives; labels int32 [2B] = ones, then
 *     zeros -- the order of the reference's torch.cat (:360-366).
 * mv_pair_assemble: one launch per batch.  Banks: txt_ids int64 [T_items, S+1] (each row tokens + [SEP] + [PAD]...), txt_len int32
 *     [T_items] (counting the [SEP]), img_feats [I_items, N, F] (dtype), img_pos int64 [I_items, N] (nullable, with pos_out);
 *     pairs int32 [R, 2] (an index outside its bank is clamped into it).  Writes input_txt int64 [R, S+1], segment int64 [R, S+1]
 *     (all ones, :203), n_ids int32 [R], desc int32 [R, 3] = {4 (1-D family), N+2, N+2+len}, feats [R, N, F] (dtype), pos_out
 *     int64 [R, N].
 * mv_rank_groups: logits f32 [G*C, 2], labels int32 [G*C] (1 = aligned), ks = HOST array of nk <= 8 positive cut-offs.
 *     p f32 [G*C] = softmax(logits)[:, 1] in f32; everything else ranks the WRITTEN p.  pos int32 [G*C] = candidates of the same
 *     group ahead of this one: descending p, exact ties by the HIGHER candidate index first, NaN after every number -- what
 *     reversing a stable ascending sort gives (np.argsort(sim)[::-1]; numpy's default sort is stable for short arrays only, so the
 *     reference's order among exact ties is otherwise unspecified, and numpy would put NaN first).  rank int32 [G] = the least pos
 *     among aligned candidates, C when none is aligned.  counters uint64 [28], ACCUMULATED (zero them first): [0] groups,
 *     [1] groups without an aligned candidate, [2] sum of fx(1 / (rank + 1)), [3] unused, [4+q] sum of [rank < k_q],
 *     [12+q] sum over groups with an aligned candidate of fx(aligned in the top k_q / aligned in the group), [20+q] sum of aligned in
 *     the top k_q (precision@k_q = that / k_q; k_q > C takes the whole group); fx(x) = rint(x * 2^32) of the f64 quotient, so the
 *     sums are integers and do not depend on the order in which groups finish.  One block per group, any C >= 1.
 * Null pointers, non-positive sizes, n < 2, C < 1, nk > 8, a cut-off <= 0: MV_E_ARG; unknown dtype: MV_E_DTYPE; D > 300 or sizes past
 * the 32-bit counters: MV_E_SHAPE.  */
int mv_pair_draws(unsigned long long key, unsigned long long step, int B, int D, uint32_t* draws, void* stream);
int mv_pair_negatives(const int32_t* idx, int B, int n, const int32_t* class_id, unsigned long long key, unsigned long long step,
                      const uint32_t* draws, int n_draws, int32_t* pairs, int32_t* labels, void* stream);
int mv_pair_assemble(const int64_t* txt_ids, const int32_t* txt_len, int T_items, const void* img_feats, int dtype, int I_items,
                     const int64_t* img_pos, const int32_t* pairs, int R, int N, int S, int F, int64_t* input_txt, int64_t* segment,
                     int32_t* n_ids, int32_t* desc, void* feats, int64_t* pos_out, void* stream);
int mv_rank_groups(const float* logits, const int32_t* labels, int G, int C, const int32_t* ks, int nk, float* p, int32_t* pos,
                   int32_t* rank, unsigned long long* counters, void* stream);

/* ---- report fine-tuning from a device-resident bank (csrc/mv_report.hip) ---------------------------------------------------
 * The reference's Preprocess4Seq2seq (Downstream_task/report_generation_and_vqa/sc/data_loader.py:330-419) from banks that live on the
 * device, and the row plan of CXRBertForReportFinetune (report_finetune.build_plan) without the host.  Additive entry points.
 *
 * mv_report_draws: the masking draw's random words.  draws uint32 [B, T+1]: word (i, t) = the counter-based hash keyed by (key, step)
 *     -- one stream per pair, derived as mv_pair_draws derives it -- at counter i (T+1) + t.  Words t < T are the shuffle keys of text
 *     index t, word T is the coin.
 * mv_report_assemble: one launch per batch.  Banks: txt_ids int64 [n_items, T] (each row tokens + [SEP] + [PAD]...), txt_len int32
 *     [n_items] (counting the [SEP]; clamped to [1, T]), n_pred int32 [n_items], img_feats [n_items, N, F] (dtype), img_pos int64
 *     [n_items, N].  Per batch: idx int32 [B] (an index outside the bank is clamped into it), family int32 [B] (nullable = 1, the
 *     seq2seq family), draws uint32 [B, T+1] (nullable; replaces the hash).  For slot i with item d = idx[i], len = txt_len[d] and
 *     p = min(n_pred[d], max_pred, len): the candidates are the text indices 0 .. len-1 (the last is the [SEP]); the rank of t is the
 *     number of candidates t' with (word[t'], t') < (word[t], t) -- equal words go to the lower index; coin = the top bit of word T.
 *     coin set: slots 0 .. p-2 list the indices of ranks 0 .. p-2 and slot p-1 lists index len-1 (so the [SEP] can be listed twice,
 *     data_loader.py:357-360); else slots 0 .. p-1 list ranks 0 .. p-1.  A slot that lists index t holds masked_pos = N + 2 + t,
 *     masked_lm_labels = txt_ids[d, t], masked_weights = 1; slots p .. max_pred-1 hold (0, 0, 0).
 *     Writes input_txt int64 [B, T] (the bank row with 103 = [MASK] at every listed index), segment int64 [B, T] (1 for t < len, else
 *     0), desc int32 [B, 3] = {family, N+2, N+2+len}, feats [B, N, F] (dtype), pos_out int64 [B, N], masked_pos / masked_lm_labels
 *     int64 [B, max_pred], masked_weights f32 [B, max_pred].  T <= 1024, max_pred <= 64.
 * mv_report_plan: the prediction lists -> the distinct consumed rows and the entries in CSR form over them (what mv_lm_loss_* and the
 *     encoder's consumed-rows last layer take).  pos / labels int64 [B, P], weights f32 [B, P], valid_len int32 [B] (nullable; packed
 *     rows).  A slot of weight 0 is dropped.  Any other slot is BAD when its weight is negative or not finite, its position is <= 0,
 *     >= L or >= valid_len[b], or its label lies outside [0, V): it is counted and left out.  The others are the entries.
 *     rows int32 [U] = the distinct b L + pos, ascending; row_ptr int32 [U+1] (row_ptr[U] = n); labels int32 [n], weights f32 [n],
 *     sample int32 [n]: grouped by row, in slot order inside a row; counts int32 [4] = {U, n, bad, 0}.  Every output array holds
 *     B P elements (row_ptr one more); elements past U / n are not written.  work: int32 [3 B] scratch.  Two launches (one wave per
 *     sample: count, then offsets and write), no atomics: fully defined and bitwise reproducible.  P <= 64, B <= 2048, B L < 2^31.
 * Null pointers (family, draws, valid_len excepted), non-positive sizes: MV_E_ARG; unknown dtype: MV_E_DTYPE; beyond the limits above
 * or the 32-bit hash counters (B (T+1) >= 2^30): MV_E_SHAPE.  */
int mv_report_draws(unsigned long long key, unsigned long long step, int B, int T, uint32_t* draws, void* stream);
int mv_report_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* n_pred, int n_items, const void* img_feats,
                       int dtype, const int64_t* img_pos, const int32_t* idx, const int32_t* family, int B, int N, int T, int F,
                       int max_pred, unsigned long long key, unsigned long long step, const uint32_t* draws, int64_t* input_txt,
                       int64_t* segment, int32_t* desc, void* feats, int64_t* pos_out, int64_t* masked_pos, int64_t* masked_lm_labels,
                       float* masked_weights, void* stream);
int mv_report_plan(const int64_t* pos, const int64_t* labels, const float* weights, const int32_t* valid_len, int B, int P, int L, int V,
                   int32_t* work, int32_t* rows, int32_t* row_ptr, int32_t* out_labels, float* out_weights, int32_t* out_sample,
                   int32_t* counts, void* stream);

/* ---- VQA fine-tuning and evaluation from a device-resident question bank (csrc/mv_vqa_bank.hip) ------------------------------
 * The reference's VQA-RAD loader (Downstream_task/report_generation_and_vqa/sc/data_loader.py:236-273: many questions per image, a
 * sparse soft answer per question), its Preprocess4Seq2seq for questions (:340-392) and the score of compute_score_with_logits
 * (pytorch_pretrained_bert/model.py:1007-1023).  Additive entry points.
 *
 * The bank: txt_ids int64 [n_questions, T] (each row tokens + [SEP] + [PAD]...), txt_len int32 [n_questions] (counting the [SEP];
 *     clamped to [1, T]), q_img int32 [n_questions] (the question's image; clamped to [0, n_images)), the answers in CSR form --
 *     ans_ptr int32 [n_questions + 1], ans_label int32 [nnz], ans_score f32 [nnz] (both nullable when nnz = 0; offsets are clamped to
 *     [0, nnz]) --, ans_type int32 [n_questions] (0 closed, 1 open, anything else neither), img_feats [n_images, N, F] (dtype),
 *     img_pos int64 [n_images, N].
 * mv_vqa_assemble: one launch per batch, grid (B, chunks of the N F feature row).  idx int32 [B] (an index outside the bank is clamped
 *     into it), family int32 [B] (nullable = 4, the 1-D family).  For slot i with question d = idx[i], image m = q_img[d] and
 *     len = txt_len[d] it writes input_txt int64 [B, T] (the bank row as it is: VQA masks nothing), segment int64 [B, T] (1 for
 *     t < len, else 0), desc int32 [B, 3] = {family, N+2, N+2+len}, feats [B, N, F] (dtype) = img_feats[m] bit for bit, pos_out int64
 *     [B, N] = img_pos[m], target f32 [B, A] = zeros with target[i, ans_label[e]] = ans_score[e] for e = ans_ptr[d] .. ans_ptr[d+1]-1
 *     in that order (a later duplicate of a label wins, as target.scatter_(0, labels, scores) on the CPU; a label outside [0, A) is
 *     skipped), ans_type_out int32 [B] = ans_type[d].  No atomics: fully defined and bitwise reproducible.  T <= 1024, N F < 2^31,
 *     B T < 2^31.
 * mv_vqa_score: pred int64 [B] (an answer column: arg_train or arg_infer of mv_bce_fwd_bwd), idx int32 [B] (clamped), group int32
 *     [n_questions] (nullable = group 0; clamped to [0, G)), G <= 8.  s = ans_score of the LAST entry of question idx[i] whose label
 *     equals pred[i], else 0: the dense target's value at the predicted column.  score f32 [B] (nullable) = s.  counters uint64
 *     [G, 3, 2], ACCUMULATED (zero them first): for the sample's group g and type slot t (0 closed, 1 open, 2 neither) it adds
 *     {fx(s), 1} to counters[g, t]; fx(x) = rint(x * 2^32) of the value widened to f64 (two's complement when negative), so the sums
 *     are integers and do not depend on the order in which samples finish.
 * Null pointers (family, group, score, and ans_label / ans_score at nnz = 0, excepted), non-positive sizes, nnz < 0: MV_E_ARG; unknown
 * dtype: MV_E_DTYPE; G > 8, T > 1024, N F or B T past 32-bit indexing: MV_E_SHAPE.  All of it is checked before anything touches the
 * HIP runtime.  */
int mv_vqa_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* q_img, int n_questions, const int32_t* ans_ptr,
                    const int32_t* ans_label, const float* ans_score, int nnz, const int32_t* ans_type, const void* img_feats, int dtype,
                    const int64_t* img_pos, int n_images, const int32_t* idx, const int32_t* family, int B, int N, int T, int F, int A,
                    int64_t* input_txt, int64_t* segment, int32_t* desc, void* feats, int64_t* pos_out, float* target,
                    int32_t* ans_type_out, void* stream);
int mv_vqa_score(const int64_t* pred, const int32_t* idx, int B, int n_questions, const int32_t* ans_ptr, const int32_t* ans_label,
                 const float* ans_score, int nnz, const int32_t* ans_type, const int32_t* group, int G, float* score,
                 unsigned long long* counters, void* stream);

/* ---- diagnosis classification from a device-resident bank (csrc/mv_clf_bank.hip) -------------------------------------------
 * The reference's JsonlDataset + collate_fn (Downstream_task/Classification/mmbt/data/dataset.py:36-85, data/helpers.py:73-98) and
 * the counts behind model_eval's metrics (mmbt/main.py:138-193).  Additive entry points.
 *
 * The bank: txt_ids int64 [n_samples, T] (each row tokens + [SEP] + [PAD]...), txt_len int32 [n_samples] (counting the [SEP]), s_img
 *     int32 [n_samples] (the image of a sample; clamped into the image bank), lab_bits int32 [n_samples, W], W = ceil(C / 32): class c
 *     is bit c % 32 of word c / 32, img_feats [n_images, N, F] (dtype), img_pos int64 [n_images, N].
 * mv_clf_assemble: one launch per batch, grid (B, chunks of the N F feature row).  idx int32 [B] (an index outside the bank is clamped
 *     into it), family int32 [B] (nullable = 4, the 1-D family).  For slot i with sample d = idx[i], image m = s_img[d] and
 *     len = txt_len[d] clamped to [1, T] it writes input_txt int64 [B, T] (the bank row as it is), segment int64 [B, T] (1 for t < len,
 *     else 0), desc int32 [B, 3] = {family, N+2, N+2+len}, feats [B, N, F] (dtype) = img_feats[m] bit for bit, pos_out int64 [B, N] =
 *     img_pos[m], target f32 [B, C] = 1.0 where the class's bit is set, else 0.0.  No atomics: fully defined and bitwise reproducible.
 *     T <= 1024, C <= 1024, N F < 2^31, B T < 2^31.
 * mv_clf_counts: probs f32 [n, ld] (ld >= C; the sigmoid probabilities mv_bce_multilabel writes), idx int32 [n] (the sample of each
 *     row; clamped into the n_items samples of lab_bits).  counters uint64 [C + 1, 7], ACCUMULATED (zero them first): rows 0 .. C-1
 *     one class each over the n samples, row C every one of the n C (sample, class) elements as ONE list (the micro average).  Columns
 *     {n_pos, n_neg, gt, eq, tp, fp, fn}: the elements whose label bit is set / clear; the pairs (p positive, q negative) of the list
 *     with prob_p > prob_q / prob_p == prob_q (f32 comparison; -0 equals +0; a NaN is unspecified); the elements with prob > 0.5f
 *     and the bit set (tp) or clear (fp), and those at or below with the bit set (fn).  AUROC = (2 gt + eq) / (2 n_pos n_neg), the
 *     tie-averaged rank statistic.  Integer counts, added with 64-bit integer atomics: the result does not depend on the order in
 *     which blocks finish.  Pair counting is quadratic: n C <= 2^21, C <= 1024.
 * Null pointers (family excepted), non-positive sizes, ld < C: MV_E_ARG; unknown dtype: MV_E_DTYPE; T > 1024, C > 1024, N F or B T
 * past 32-bit indexing, n C > 2^21: MV_E_SHAPE.  All of it is checked before anything touches the HIP runtime.  */
int mv_clf_assemble(const int64_t* txt_ids, const int32_t* txt_len, const int32_t* s_img, const int32_t* lab_bits, int n_samples,
                    const void* img_feats, int dtype, const int64_t* img_pos, int n_images, const int32_t* idx, const int32_t* family,
                    int B, int N, int T, int F, int C, int64_t* input_txt, int64_t* segment, int32_t* desc, void* feats,
                    int64_t* pos_out, float* target, void* stream);
int mv_clf_counts(const float* probs, int ld, const int32_t* idx, int n, const int32_t* lab_bits, int n_items, int C,
                  unsigned long long* counters, void* stream);

/* ---- corpus BLEU-1..4 of generated reports (csrc/mv_bleu.hip) ---------------------------------------------------------------
 * The reference's evaluation of report generation (Downstream_task/report_generation_and_vqa/sc/generation_decode.py:480-498,
 * detokenize :97-104, sc/bleu.py:16-64): nltk's corpus_bleu over ' '.join(detokenize(tokens)).split(' ') against
 * gt_caption.split(' ').  Additive entry points.
 *
 * Word keys: a word is named by the polynomial hash of its UTF-8 bytes modulo 2^64 with a fixed odd multiplier P (report_eval.py),
 *     key(a + b) = key(a) P^len(b) + key(b), stored as the int64 of the same bits.  Equal keys are taken for equal words.  The
 *     tables, one entry per vocabulary id: tok_key (the whole token string, with its ## where it has one), tail_key (tok[2:] of a
 *     token that starts with ##), tail_pow (P^len(tok[2:]), 0 for a token that is no continuation); empty_key = key('').
 * mv_bleu_words: ids int64 [n, T] with row stride ld >= T.  A row ends before its first eos_id or pad_id, or at T; an id outside
 *     [0, V) ends it as pad_id does.  A kept token with tail_pow != 0 that is not the row's first extends the current word (key =
 *     key tail_pow + tail_key); every other kept token starts a word with tok_key (a leading ##x keeps its ##).  A row without a kept
 *     token holds the one word empty_key.  word_key int64 [n, T]: the row's words in order, 0 behind them; n_words int32 [n].  No
 *     atomics on global memory: bitwise reproducible.  T <= 1024, V <= 2^20, n <= 2^20.
 * mv_bleu_counts: hyp_key int64 [n, Th] / hyp_n int32 [n] (mv_bleu_words' outputs; a count is clamped to [0, Th]), ref_key int64
 *     [n_items, Tr] / ref_n int32 [n_items], idx int32 [n]: row i is scored against item idx[i], clamped into the bank.  counters
 *     uint64 [10] = {num_1..num_4, den_1..den_4, hyp_len, ref_len}, ACCUMULATED (zero them first): per sample with Lh hypothesis and
 *     Lr reference words, num_o += the sum over the distinct hypothesis o-grams g of min(count_hyp(g), count_ref(g)) -- the o words
 *     compared one by one --, den_o += max(1, Lh - o + 1) (nltk's modified_precision), hyp_len += Lh, ref_len += Lr.  Integer
 *     counts added with 64-bit integer atomics: the result does not depend on the order in which blocks finish.  Th, Tr <= 1024,
 *     n <= 2^20.
 * Null pointers, non-positive sizes, ld < T: MV_E_ARG; T, Th or Tr > 1024, V > 2^20, n > 2^20: MV_E_SHAPE.  All of it is checked
 * before anything touches the HIP runtime.  */
int mv_bleu_words(const int64_t* ids, int ld, int n, int T, const int64_t* tok_key, const int64_t* tail_key, const int64_t* tail_pow,
                  int V, int64_t eos_id, int64_t pad_id, int64_t empty_key, int64_t* word_key, int32_t* n_words, void* stream);
int mv_bleu_counts(const int64_t* hyp_key, int Th, const int32_t* hyp_n, int n, const int64_t* ref_key, int Tr, const int32_t* ref_n,
                   int n_items, const int32_t* idx, unsigned long long* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEDVILL_H_ */
