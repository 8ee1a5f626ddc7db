/* libfmmt_hip -- the replica digest: six 64-bit words over the bits of every parameter and optimizer moment, for data-parallel runs that want
 * to know that every rank still holds the same state; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on
 * `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_DIGEST_H
#define FMMT_DIGEST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Data-parallel replicas start from the same bits and apply the same averaged gradients, so parameters and moments stay bit-identical on every
 * rank -- until something breaks that (a rank that skipped an update alone, a collective that was left out).  Comparing the state itself means
 * copying it to the host: 1.7 GB of parameters and 3.5 GB of moments per rank for the T+A+V model.  The digest reads them once on the device.
 *
 * fmmt_param_digest works on the descriptor table of fmmt_adamw_batch (fmmt.h: records {p, g, m, v, low, n, first block, flag} in blocks of
 * 4096 elements; n_blocks is that table's block count) and reads p, m and v of every record; g and low are not touched.  For record j
 * (0-based, table order), element i (0-based) and e = the element's 32 bits taken as an unsigned integer, per quantity:
 *     S1 = sum of e                                   mod 2^64
 *     S2 = sum of e * ((i + 1) + (j + 1) * 2^32)      mod 2^64
 * out[0], out[1] = S1, S2 of the parameters; out[2], out[3] of the first moments; out[4], out[5] of the second moments.  The sums are integer
 * sums: the result does not depend on the order of summation and is the same on every call, stream and device.  S1 changes with any single
 * changed bit; S2 also with two elements that trade places (+0.0 and -0.0 differ in both).
 *   partial: 6 * n_blocks 64-bit words of scratch, written then read by this call; out: 6 words.  Both 8-byte aligned (FMMT_EALIGN otherwise).
 *   NULL desc / partial / out, n_desc < 1 or n_blocks < 1: FMMT_EINVAL.  Both are checked before anything is launched.
 *   Two launches on `stream` (one workgroup per block, then one workgroup that sums the blocks' words); no atomics, capture-safe. */
int fmmt_param_digest(int n_desc, int n_blocks, const void* desc, uint64_t* partial, uint64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
