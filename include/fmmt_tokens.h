/* libfmmt_hip -- the text encoder on real tokens only; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on
 * `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_TOKENS_H
#define FMMT_TOKENS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A MELD text batch is B dialogues padded on the right to T tokens (utils/dataset.py: input_ids / input_mask; src/models.py:95-107 runs the encoder
 * on all B * T rows).  A padded token is masked as a key and never read as a query (src/models.py:112-150 gathers target-utterance tokens), so the
 * encoder's layers can run on the real rows alone: the rows of sequence b packed at [off[b], off[b] + len[b]) of a buffer of a FIXED number of rows
 * `cap` (a captured HIP graph keeps one shape), zeros behind the last sequence.  These entry points are what that needs beside fmmt_pack_frames
 * (fmmt_ragged.h), which packs (B, T, row_bytes) by per-row counts as it is.
 *
 * fmmt_token_layout: mask [B][T] int32 (non-zero = real token) -> the packing of its rows' leading real tokens, one launch of one workgroup:
 *   len [B] int32 = leading non-zeros of row b, cut so that off[b] + len[b] <= cap; off [B] int32 = len[0] + ... + len[b-1]; len64 [B] int64 = len
 *   (the counts fmmt_pack_frames / fmmt_unpack_rows take); row_map [cap] int32: packed row r of sequence b, token t -> b * T + t, its row in the
 *   padded layout; a row behind the last sequence -> B * T + r (no padded row has that index); counts [2] int32 = {rows packed, non-zeros of the
 *   mask}: counts[1] != counts[0] tells the caller that the mask has a hole or does not fit `cap`.  B <= 256, T <= 65535, cap <= 65535, else FMMT_EINVAL.
 *
 * fmmt_unpack_rows: the inverse of fmmt_pack_frames.  src [cap][row_bytes], counts [B] int64 (device; clamped to [0, L]) -> dst [B][L][row_bytes]:
 *   row (u, k) = src[n_0 + ... + n_{u-1} + k] for k < n_u and a source row below cap, zeros elsewhere (every byte of dst is written).  Each is the
 *   other's backward: the gradient of the packed rows is the pack of the padded gradient, the gradient of the padded rows the unpack of the packed one.
 *   Limits and alignment as fmmt_pack_frames (B <= 256, B * L <= 2^31 - 1, row_bytes % 16 == 0).
 *
 * fmmt_mha_fwd_ragged / fmmt_mha_bwd_ragged: fmmt_mha_fwd / _bwd (fmmt.h) | FMMT_BATCH_MAJOR for self-attention on packed rows -- dtype = FMMT_BF16 |
 *   FMMT_RAGGED, head_dim 64, the matrix-core kernels (anything else: FMMT_EINVAL; leading dimensions % 8).  q / k / v / out / dout / dq / dk / dv hold
 *   `rows` rows; sequence b's are [seq_off[b], seq_off[b] + seq_len[b]) (device int32 [B], sequences back to back from row 0 as fmmt_token_layout
 *   writes them; a length is cut to T and to the rows the operands hold, so no access leaves them).  T is the PADDED length: the grid, lse's
 *   layout [B][num_heads][T] and the dropout counters (query row (b * num_heads + head) * T + t, key groups of T) are those of the padded call, so
 *   out / lse / dq / dk / dv of the real rows are bit for bit what fmmt_mha_* | FMMT_BATCH_MAJOR on (B, T) computes with key_bias = -30000 on the padded
 *   keys and zero dout on the padded queries: a key past seq_len takes the "past the last key" term, a workgroup whose first query (key) is past it exits.
 *   lse[b][h][t >= seq_len[b]] is not written.  Rows [seq_off[B-1] + seq_len[B-1], rows) of out / dq / dk / dv are ZERO-FILLED (the GEMMs around the
 *   attention contract over them); rows <= B * T.
 *
 * fmmt_dropadd_ln_fwd_map / _bwd_map: fmmt_dropadd_ln_fwd / _bwd (fmmt.h) with row_map [M] int32 (or NULL: the same as those): row r draws the dropout
 *   mask of row row_map[r] -- the map only enters the counter row * C + column of the generator --, so the call on packed rows keeps, bit for bit, the
 *   elements the call on the padded layout keeps.  Everything else (operands, workspace, summation order over the M rows given) is unchanged. */
#define FMMT_RAGGED 0x800
int fmmt_token_layout(int B, int T, int cap, const int32_t* mask, int32_t* seq_len, int32_t* seq_off, int64_t* len64, int32_t* row_map,
                      int32_t* counts, void* stream);
int fmmt_unpack_rows(int B, int L, int cap, size_t row_bytes, const void* src, const int64_t* counts, void* dst, void* stream);
int fmmt_mha_fwd_ragged(int dtype, int T, int B, int E, int num_heads, int rows, const int32_t* seq_off, const int32_t* seq_len,
                        const void* q, int ldq, const void* k, const void* v, int ldkv, float scale,
                        float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out, int ldo, float* lse, void* stream);
int fmmt_mha_bwd_ragged(int dtype, int T, int B, int E, int num_heads, int rows, const int32_t* seq_off, const int32_t* seq_len,
                        const void* q, int ldq, const void* k, const void* v, int ldkv, float scale,
                        float dropout_p, uint64_t seed, const uint64_t* seed_dev, const void* out, const void* dout, int ldo,
                        const float* lse, void* dq, int lddq, void* dk, void* dv, int lddkv, void* stream);
int fmmt_dropadd_ln_fwd_map(int param_dtype, int M, int C, float eps, const void* h, const void* res, const void* gamma, const void* beta, float p,
                            uint64_t seed, const uint64_t* seed_dev, uint64_t salt, void* xsum, void* y, const int32_t* row_map, void* stream);
int fmmt_dropadd_ln_bwd_map(int param_dtype, int M, int C, float eps, const void* dy, const void* xsum, const void* gamma, float p, uint64_t seed,
                            const uint64_t* seed_dev, uint64_t salt, void* dx, void* dh, void* dgamma, void* dbeta, void* dbias, void* workspace,
                            size_t workspace_bytes, const int32_t* row_map, void* stream);

#ifdef __cplusplus
}
#endif
#endif
