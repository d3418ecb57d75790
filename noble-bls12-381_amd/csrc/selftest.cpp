// selftest.cpp -- host-side self test of the wave VM's compiler and simulator for the sanitizer build (make debug -> nbls_selftest, built with
// -fsanitize=address,undefined).  TEST INFRASTRUCTURE (not part of libnbls.so): compiles every step program, verifies each one statically
// (verify_program), and runs the pairing of the two generators through the simulator -- Miller loop as one program and as LINES + ACC -- printing
// the first coefficient of the Miller value, which tests/test_debug_build.py compares with the reference's (SURVEY 8(c) anchor).  Also the quotient walk of fr_exec.h
// (fr_eval_lane_t<true> / fr_quot_lane: the host side of kzg_quotient_kernel) on heap blocks of exactly the call's sizes, off a root and on one, and the transform, the cells
// and the quotient rows of the cell proofs (fr_ntt_* / fr_cell_chain: the host side of kzg_ntt_kernel and kzg_cell_rows_kernel) likewise.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "programs.h"
#include "consts_gen.h"
#include "vm_exec.h"

extern "C" int nbls_sim_run(int prog, unsigned n_items, uint8_t** ptrs, const uint64_t* strides);
extern "C" int nbls_sim_extra_run_named(const char* name, int aot, unsigned n_items, uint8_t** ptrs, const uint64_t* strides);
extern "C" void nbls_sim_set_aot(int on);
extern "C" int nbls_sim_fr_eval_roots(unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out32, int8_t* status);
extern "C" int nbls_sim_fr_quotient_roots(unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out_y32, uint8_t* out_q32, int8_t* status);
extern "C" int nbls_sim_fr_ntt(unsigned log2_n, int dir, size_t n, const uint8_t* in32, const uint8_t* shift32, uint8_t* out32, int8_t* status);
extern "C" int nbls_sim_kzg_cells(unsigned log2_n, size_t n, const uint8_t* blobs, uint8_t* out_cells, uint8_t* coef32, int8_t* status);
extern "C" int nbls_sim_kzg_cell_rows(unsigned log2_n, unsigned log2_cell, size_t n, const uint8_t* coef32, uint8_t* out_q32);
extern "C" int nbls_sim_kzg_cell_interp(unsigned log2_n, unsigned log2_cell, size_t n_cells, int sum, unsigned n_wg, const uint8_t* cells, const uint32_t* cell_index,
                                        const int8_t* pre, const uint8_t* w32, uint8_t* out, int8_t* st_out);
extern "C" int nbls_sim_kzg_recover(unsigned log2_n, unsigned log2_cell, size_t n, const uint32_t* cell_offsets, const uint32_t* cell_index, const uint8_t* cells,
                                    uint8_t* out_cells, uint8_t* coef32, int8_t* status);
extern "C" int nbls_sim_g16_input_sums(size_t n, size_t m, unsigned n_wg, const uint8_t* inputs32, const uint8_t* weights32, const int8_t* pre, uint8_t* out32, int8_t* status);
using namespace nbls;

static void be48(uint8_t* o, const u32* limbs) { u32 w[12]; limbs_to_words(w, limbs); for (int i = 0; i < 12; i++) { u32 v = w[11 - i]; o[4 * i] = v >> 24; o[4 * i + 1] = v >> 16; o[4 * i + 2] = v >> 8; o[4 * i + 3] = v; } }

int main() {
  int bad = 0;
  for (int i = 0; i < P_COUNT; i++) {
    const Program& p = get_program((ProgId)i);
    const std::string e = verify_program(p);
    if (!e.empty()) { printf("VERIFY FAILED %s\n", e.c_str()); bad++; }
  }
  for (int i = 0; i < XP_COUNT; i++) {
    const std::string e = verify_program(get_extra_program((ExtraProg)i));
    if (!e.empty()) { printf("VERIFY FAILED %s\n", e.c_str()); bad++; }
  }
  printf("programs %d verified, failures %d\n", (int)P_COUNT + (int)XP_COUNT, bad);
  // pairing(G1, G2, false): generators in wire form
  uint8_t g1[96], g2[192], out1[576], out2[576];
  be48(g1, NBLS_G1X_RAW); be48(g1 + 48, NBLS_G1Y_RAW);
  static const char* G2HEX = "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
                             "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                             "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"
                             "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be";   // the G2 generator (CURVE.G2x, CURVE.G2y)
  for (int i = 0; i < 192; i++) { unsigned v; sscanf(G2HEX + 2 * i, "%2x", &v); g2[i] = (uint8_t)v; }
  {
    uint8_t* ptrs[8] = {g1, g2, out1, nullptr, nullptr, nullptr, nullptr, nullptr}; uint64_t strides[8] = {96, 192, 576, 0, 0, 0, 0, 0};
    if (nbls_sim_run(P_MILLER_BYTES, 1, ptrs, strides)) return 2;
  }
  {
    std::vector<uint8_t> lines((size_t)LINE_ELEMS * RAW_FP_BYTES);
    uint8_t* ptrs[8] = {g1, g2, out2, lines.data(), nullptr, nullptr, nullptr, nullptr}; uint64_t strides[8] = {96, 192, 576, lines.size(), 0, 0, 0, 0};
    if (nbls_sim_run(P_LINES_PQ, 1, ptrs, strides) || nbls_sim_run(P_ACC_BYTES, 1, ptrs, strides)) return 2;
  }
  {
    // the line program of the calls that end in a final exponentiation, interpreted and translated, into a table of exactly LINE_ELEMS elements, then the accumulation and FE_FINAL
    // in its translated form (the chain of nine factors) on that value seven times over: memory safety of the new programs' loads and stores; what they compute is the tests' matter
    std::vector<uint8_t> lines((size_t)LINE_ELEMS * RAW_FP_BYTES), F(12 * RAW_FP_BYTES), N(RAW_FP_BYTES), W(576);
    for (int aot = 0; aot < 2; aot++) {
      uint8_t* ptrs[8] = {g1, g2, nullptr, lines.data(), N.data(), F.data(), nullptr, nullptr}; uint64_t strides[8] = {96, 192, 0, lines.size(), N.size(), F.size(), 0, 0};
      nbls_sim_set_aot(aot);
      if (nbls_sim_extra_run_named("lines_fe", aot, 1, ptrs, strides) || nbls_sim_run(P_ACC_FE, 1, ptrs, strides)) return 2;
      uint8_t* tp[8] = {F.data(), F.data(), F.data(), F.data(), F.data(), F.data(), F.data(), W.data()}; uint64_t ts[8] = {F.size(), F.size(), F.size(), F.size(), F.size(), F.size(), F.size(), 576};
      if (nbls_sim_run(P_FE_FINAL, 1, tp, ts)) return 2;
    }
    nbls_sim_set_aot(0);
  }
  for (unsigned log2_n : {2u, 9u}) {   // below one term per lane, and two terms per lane; polynomial 0 at z = 5, polynomial 1 at z = 1 = w_0
    const size_t N = (size_t)1 << log2_n;
    std::vector<uint8_t> ev(2 * N * 32), z(2 * 32), y(2 * 32), y2(2 * 32), q(2 * N * 32); std::vector<int8_t> st(2);
    for (size_t i = 0; i < ev.size(); i++) ev[i] = (i % 32) ? (uint8_t)(i * 37 + 11) : 0;   // (top byte 0: canonical)
    z[31] = 5; z[63] = 1;
    if (nbls_sim_fr_quotient_roots(log2_n, 2, ev.data(), z.data(), y.data(), q.data(), st.data()) || nbls_sim_fr_eval_roots(log2_n, 2, ev.data(), z.data(), y2.data(), nullptr)) return 2;
    if (st[0] || st[1] || memcmp(y.data(), y2.data(), 64) || memcmp(y.data() + 32, ev.data() + N * 32, 32)) { printf("QUOTIENT: y differs from the evaluation\n"); bad++; }
  }
  printf("quotient walk ok\n");
  for (unsigned log2_n : {1u, 5u, 10u}) {   // below one element per lane, and two: the transform there and back with a shift, the cells, the quotient rows of one-element and of whole-blob cells
    const size_t N = (size_t)1 << log2_n;
    std::vector<uint8_t> ev(2 * N * 32), sh(2 * 32), co(2 * N * 32), back(2 * N * 32), cells(2 * 2 * N * 32), co2(2 * N * 32); std::vector<int8_t> st(2);
    for (size_t i = 0; i < ev.size(); i++) ev[i] = (i % 32) ? (uint8_t)(i * 29 + 5) : 0;
    sh[31] = 3; sh[63] = 7;
    if (nbls_sim_fr_ntt(log2_n, 0, 2, ev.data(), sh.data(), co.data(), st.data()) || nbls_sim_fr_ntt(log2_n, 1, 2, co.data(), sh.data(), back.data(), nullptr)) return 2;
    if (st[0] || st[1] || back != ev) { printf("NTT: the round trip differs\n"); bad++; }
    if (nbls_sim_kzg_cells(log2_n, 2, ev.data(), cells.data(), co2.data(), st.data()) || nbls_sim_fr_ntt(log2_n, 0, 2, ev.data(), nullptr, co.data(), nullptr)) return 2;
    if (st[0] || st[1] || co2 != co || memcmp(cells.data(), ev.data(), N * 32) || memcmp(cells.data() + 2 * N * 32, ev.data() + N * 32, N * 32)) { printf("CELLS: coefficients or blob bytes differ\n"); bad++; }
    for (unsigned log2_cell : {0u, log2_n}) {
      std::vector<uint8_t> q((size_t)2 * ((2 * N) >> log2_cell) * N * 32);
      if (nbls_sim_kzg_cell_rows(log2_n, log2_cell, 2, co.data(), q.data())) return 2;
    }
    // the verifier's interpolation of whole-blob cells (c = N <= 64): three cells, the rows mode against the sum mode of each cell alone with weight one, over two workgroups
    if (log2_n <= 6) {
      const uint32_t idx[3] = {0, 1, 0};
      std::vector<uint8_t> rows(3 * N * 32), sum(N * 32), one(32); std::vector<int8_t> cst(3, 1);
      one[31] = 1;
      if (nbls_sim_kzg_cell_interp(log2_n, log2_n, 3, 0, 0, cells.data(), idx, nullptr, nullptr, rows.data(), cst.data())) return 2;
      if (cst[0] || cst[1] || cst[2]) { printf("CELL INTERP: a status is set\n"); bad++; }
      for (size_t k = 0; k < 3; k++) {
        if (nbls_sim_kzg_cell_interp(log2_n, log2_n, 1, 1, 2, cells.data() + k * N * 32, idx + k, nullptr, one.data(), sum.data(), nullptr)) return 2;
        if (memcmp(sum.data(), rows.data() + k * N * 32, N * 32)) { printf("CELL INTERP: the sum of one cell differs from its row\n"); bad++; }
      }
    }
    // the recovery: blob 0 from the odd cells in descending order, a refused blob (one cell short) behind it, blob 1 from all of its cells; one-element and whole-blob cells
    for (unsigned log2_cell : {0u, log2_n}) {
      const size_t M = (2 * N) >> log2_cell, cb = (size_t)32 << log2_cell;
      std::vector<uint32_t> off{0}, idx; std::vector<uint8_t> given, rec(3 * 2 * N * 32), rco(3 * N * 32); std::vector<int8_t> rst(3);
      auto give = [&](size_t blob, uint32_t k) { idx.push_back(k); given.insert(given.end(), cells.begin() + blob * 2 * N * 32 + k * cb, cells.begin() + blob * 2 * N * 32 + (k + 1) * cb); };
      for (size_t k = M; k-- > 0;) if (k & 1) give(0, (uint32_t)k);
      off.push_back((uint32_t)idx.size());
      for (size_t k = 0; k + 1 < M / 2; k++) give(0, (uint32_t)k);
      off.push_back((uint32_t)idx.size());
      for (size_t k = 0; k < M; k++) give(1, (uint32_t)k);
      off.push_back((uint32_t)idx.size());
      if (nbls_sim_kzg_recover(log2_n, log2_cell, 3, off.data(), idx.data(), given.data(), rec.data(), rco.data(), rst.data())) return 2;
      if (rst[0] || rst[1] != 22 || rst[2] || memcmp(rec.data(), cells.data(), 2 * N * 32) || memcmp(rec.data() + 4 * N * 32, cells.data() + 2 * N * 32, 2 * N * 32) ||
          memcmp(rco.data(), co.data(), N * 32) || memcmp(rco.data() + 2 * N * 32, co.data() + N * 32, N * 32)) { printf("RECOVER: cells, coefficients or statuses differ\n"); bad++; }
    }
  }
  printf("transform, cell rows, cell interpolation and recovery ok\n");
  // the weighted input sums of Groth16 in buffers of exactly the call's sizes: one tile and its last lane (m = 63), two tiles with one element in the second (m = 64), three
  // (m = 129); rows below, at and above a workgroup's 64; weight one, so that column 0 is the number of rows that are in; row 1 out beforehand
  for (size_t m : {(size_t)1, (size_t)63, (size_t)64, (size_t)129}) for (size_t n : {(size_t)2, (size_t)64, (size_t)65}) {
    std::vector<uint8_t> x(n * m * 32), w(n * 32), out((m + 1) * 32); std::vector<int8_t> pre(n), st(n, 1);
    for (size_t i = 0; i < x.size(); i++) x[i] = (i % 32) ? (uint8_t)(i * 41 + 3) : 0;   // (top byte 0: canonical)
    for (size_t i = 0; i < n; i++) w[32 * i + 31] = 1;
    pre[1] = 13;
    if (nbls_sim_g16_input_sums(n, m, 0, x.data(), w.data(), pre.data(), out.data(), st.data()) || nbls_sim_g16_input_sums(n, m, 3, x.data(), w.data(), nullptr, out.data(), nullptr)) return 2;
    if (out[31] != n || st[0] || st[1] != 13) { printf("G16 SUMS: the count of rows or a status differs\n"); bad++; }
  }
  printf("groth16 input sums ok\n");
  if (memcmp(out1, out2, 576)) { printf("MISMATCH between the fused and the split Miller loop\n"); bad++; }
  printf("miller c0.c0.c0 ");
  for (int i = 0; i < 48; i++) printf("%02x", out1[i]);
  printf("\n");
  return bad ? 1 : 0;
}
