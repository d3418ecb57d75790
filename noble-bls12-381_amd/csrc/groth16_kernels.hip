// groth16_kernels.hip -- the scalar-field side of Groth16 batch verification (pipelines_groth16.cpp): the n x m matrix of public inputs folded with the weights into m + 1
// scalars (g16_input_sums_kernel, g16_sum_kernel; the lane code is fr_exec.h's, shared with the simulator: nbls_sim_g16_input_sums), and the small kernels around the decoders,
// the sums and the per-proof pass.  The curve arithmetic runs as step programs (decoders, ladders, MSMs, Miller loops).  Every store is a plain C++ vector or byte store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_workgroup.h"   // fr_exec.h, nbls.h; the tree and the closing sum
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

constexpr int GL = G16_LANES;

// fr_exec.h has the walk.  inputs: n rows of m elements; w32: n weights; pre (may be NULL): a row with pre[i] != 0 is out; partial: one row of m + 1 plain-limb elements per
// workgroup of rows (wgs of them); st_out (may be NULL): the rows' statuses, written by tile 0.
// Grid: one dimension, ceil(wgs / 8) * 8 * tiles workgroups, dealt so that the `tiles` workgroups of one set of rows are 8 apart: workgroups b and b + 8 run on the same XCD,
// so the tiles of a row, each of which looks at the whole row, meet in that XCD's L2 and the matrix comes from memory once (with the tiles as blockIdx.x of a 2-D grid they
// fell on different XCDs: 92 us at 8192 x 328, six times the matrix at the rate of memory).  For speed only: no answer depends on where a workgroup runs
__global__ void __launch_bounds__(GL) g16_input_sums_kernel(u32 n, u32 m, u32 wgs, const uint8_t* __restrict__ inputs, const uint8_t* __restrict__ w32, const int8_t* __restrict__ pre,
                                                            Fr* __restrict__ partial, int8_t* __restrict__ st_out) {
  __shared__ Fr part[GL];
  const u32 t = threadIdx.x, lane = t & (G16_TILE - 1), tiles = g16_tiles(m), span = 8 * tiles, r = blockIdx.x % span, tile = r / 8, wg = blockIdx.x / span * 8 + r % 8;
  if (wg >= wgs) return;   // (the whole workgroup: the last eight may be fewer)
  const u32 groups = wgs * G16_GROUPS, q = wg * G16_GROUPS + t / G16_TILE;
  G16Acc acc = g16_acc_zero();
  for (u64 i = q; i < n; i += groups) {   // (the same rows on every lane of a wavefront)
    u32 bad;
    const Fr x = g16_row_lane(inputs + i * m * 32, m, tiles, tile, lane, &bad);
    bad = __any((int)bad) ? 0xffffffffu : 0u;
    const int p = pre ? pre[i] : 0;
    g16_row_add(acc, x, w32 + 32ull * i, bad | ((u32)0 - (u32)(p != 0)));
    if (st_out && tile == 0 && lane == 0) st_out[i] = (int8_t)g16_row_status(p, bad);
  }
  const FrWorkgroup<GL> lanes;
  lanes.phase([&](u32 l) { part[l] = g16_reduce(acc); });
  fr_tree(lanes, part, G16_TILE);   // (every wavefront meets every barrier)
  const u32 c = tile * G16_TILE + t;
  if (t < G16_TILE && c <= m) partial[(u64)wg * (m + 1) + c] = part[t];
}
// out32[c] = the sum over the n_parts partial rows of column c as 32 bytes big-endian, c <= m: one workgroup per tile, row group g on the rows g, g + G16_GROUPS, ..
__global__ void __launch_bounds__(GL) g16_sum_kernel(u32 m, u32 n_parts, const Fr* __restrict__ partial, uint8_t* __restrict__ out32) {
  __shared__ Fr part[GL];
  g16_sum_body(FrWorkgroup<GL>(), m, blockIdx.x, n_parts, partial, out32, part);
}

// a proof is A || B || C (192 bytes = twelve 16-byte vectors): A to ac48[i], C to ac48[n + i] -- one array for one decoder call -- and B to b96[i]; one vector per thread
__global__ void g16_split_kernel(u32 n, const uint4* __restrict__ proofs, uint4* __restrict__ ac48, uint4* __restrict__ b96) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * 12) return;
  const VecPart v = vec_split(t, 12);
  const uint4 x = proofs[t];
  if (v.part < 3) ac48[v.elem * 3 + v.part] = x;
  else if (v.part < 9) b96[v.elem * 6 + v.part - 3] = x;
  else ac48[((u64)n + v.elem) * 3 + v.part - 9] = x;
}
// pre0[i]: what the three decoders say about proof i -- A's status if >= 1 (1: the zero point), else 10 + B's, else NBLS_ST_G16_C + C's, else 0
__global__ void g16_pre_kernel(u32 n, const int8_t* __restrict__ sta, const int8_t* __restrict__ stb, const int8_t* __restrict__ stc, int8_t* __restrict__ pre0) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = sta[i], b = stb[i], c = stc[i];
  pre0[i] = (int8_t)(a ? a : b ? 10 + b : c ? NBLS_ST_G16_C + c : 0);
}
// A proof that is out (pre[i] != 0) gets the scalar zero in the sum over the C_i, and its three points are replaced by fixed points of the subgroups (gen96: a G1 point,
// g2_192: a G2 point), so that the ladders, the MSM and the Miller loops read points of the curves only; one proof per thread.  s1[i] = r_i where the proof is in
__global__ void g16_items_kernel(u32 n, const int8_t* __restrict__ pre, const uint8_t* __restrict__ w32, const uint4* __restrict__ gen96, const uint4* __restrict__ g2_192,
                                 uint4* __restrict__ a96, uint4* __restrict__ c96, uint4* __restrict__ b192, uint4* __restrict__ s1) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool out = pre[i] != 0;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  s1[2ull * i] = out ? zero : ((const uint4*)w32)[2ull * i];
  s1[2ull * i + 1] = out ? zero : ((const uint4*)w32)[2ull * i + 1];
  if (!out) return;
  for (u32 k = 0; k < 6; k++) { a96[6ull * i + k] = gen96[k]; c96[6ull * i + k] = gen96[k]; }
  for (u32 k = 0; k < 12; k++) b192[12ull * i + k] = g2_192[k];
}
// the rows of the per-proof pass: the m inputs of a proof that is out become zeros (an element >= r is nothing the MSM's split may read); one 16-byte vector per thread
__global__ void g16_rows_kernel(u32 n, u32 m, const int8_t* __restrict__ pre, uint4* __restrict__ rows) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * m * 2) return;
  if (pre[t / (2ull * m)]) rows[t] = make_uint4(0, 0, 0, 0);
}
// the per-proof verdicts: pre[i] if != 0, else 0 where the product is one, else NBLS_ST_NOT_VERIFIED
__global__ void g16_status_kernel(u32 n, const int8_t* __restrict__ pre, const uint8_t* __restrict__ one, int8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  status[i] = pre[i] ? pre[i] : one[i] ? 0 : NBLS_ST_NOT_VERIFIED;
}
// nbls_groth16_prepare_inputs' closing: status 0, 1 where L_i is the zero point (bytes 0xc0 00..) or the row's own (48 zero bytes); one point per thread
__global__ void g16_prepare_tail_kernel(u32 n, const int8_t* __restrict__ zero, const int8_t* __restrict__ pre, uint8_t* __restrict__ out48, int8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int st = pre[i] ? pre[i] : zero[i] == 1 ? 1 : 0;
  close_compressed(out48 + 48ull * i, 48, st);
  status[i] = (int8_t)st;
}
}  // namespace

extern "C" {
// n rows of m inputs (inputs, w32, partial and out32 16-byte aligned; partial: g16_workgroups(n) * (m + 1) elements) -> out32: the m + 1 sums; st_out and pre may be NULL
int nbls_g16_input_sums_launch(unsigned n, unsigned m, const void* inputs32, const void* w32, const void* pre, void* partial, void* out32, void* st_out, hipStream_t stream) {
  if (!n || !m) return 0;
  const u32 wgs = g16_workgroups(n), tiles = g16_tiles(m);
  hipLaunchKernelGGL(g16_input_sums_kernel, dim3((wgs + 7) / 8 * 8 * tiles), dim3(GL), 0, stream, n, m, wgs, (const uint8_t*)inputs32, (const uint8_t*)w32, (const int8_t*)pre, (Fr*)partial,
                     (int8_t*)st_out);
  const int e = (int)hipGetLastError();
  return e ? e : launch_1d(g16_sum_kernel, (u64)tiles * GL, GL, 0, stream, m, wgs, partial, out32);
}
int nbls_g16_split_launch(unsigned n, const void* proofs192, void* ac48, void* b96, hipStream_t stream) {
  return launch_1d(g16_split_kernel, (u64)n * 12, 256, 0, stream, n, proofs192, ac48, b96);
}
int nbls_g16_pre_launch(unsigned n, const void* sta, const void* stb, const void* stc, void* pre0, hipStream_t stream) {
  return launch_1d(g16_pre_kernel, n, 256, 0, stream, n, sta, stb, stc, pre0);
}
int nbls_g16_items_launch(unsigned n, const void* pre, const void* w32, const void* gen96, const void* g2_192, void* a96, void* c96, void* b192, void* s1, hipStream_t stream) {
  return launch_1d(g16_items_kernel, n, 256, 0, stream, n, pre, w32, gen96, g2_192, a96, c96, b192, s1);
}
int nbls_g16_rows_launch(unsigned n, unsigned m, const void* pre, void* rows32, hipStream_t stream) {
  return launch_1d(g16_rows_kernel, (u64)n * m * 2, 256, 0, stream, n, m, pre, rows32);
}
int nbls_g16_status_launch(unsigned n, const void* pre, const void* one, void* status, hipStream_t stream) {
  return launch_1d(g16_status_kernel, n, 256, 0, stream, n, pre, one, status);
}
int nbls_g16_prepare_tail_launch(unsigned n, const void* zero, const void* pre, void* out48, void* status, hipStream_t stream) {
  return launch_1d(g16_prepare_tail_kernel, n, 256, 0, stream, n, zero, pre, out48, status);
}
}
