// vm_sim.cpp -- host-side simulator of the wave VM.  TEST INFRASTRUCTURE: lets the CPU test-suite check the
// compiled step programs (scheduler, slot allocation, descriptors, limb arithmetic) against oracle/ without a
// GPU.  It is built into libnbls_sim.so, which only tests/ load; libnbls.so (the product) does not contain it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "programs.h"
#include "vm_exec.h"
#include "consts_gen.h"
#include "fp_inv.h"
#include "pow_exec.h"
#include "pow_wide.h"
#include "rlc_weights.h"
#include "fr_workgroup.h"
#include "g16p_exec.h"
#include <algorithm>
#include "wide_exec.h"
#include "g1_wide.h"
#include "fp_inv_wide.h"
#include "scalar_split.h"
#include "aot_exec.h"
#include "aot_layout.h"
#include "aot_sigs.inc"

using namespace nbls;

static void sim_run(const Program& p, unsigned n_items, const IOBuf* bufs) {
  const u32* qp_table = qp_table_words();
  const unsigned inst_bytes = p.inst_bytes();
  std::vector<V4> lds4((size_t)p.lds_bytes() / 16 + 1);
  char* lds = (char*)lds4.data();
  unsigned blocks = (n_items + p.G - 1) / p.G;
  for (unsigned blk = 0; blk < blocks; blk++) {
    memset(lds, 0xde, (size_t)p.lds_bytes());
    for (unsigned g = 0; g < (p.shared_consts ? 1u : p.G); g++) for (unsigned c = 0; c < p.nconst; c++) memcpy(lds + g * inst_bytes + c * p.slot_bytes, p.consts.data() + c * RAW_WORDS, NL * 4);
    for (size_t s = 0; s < p.steps.size(); s++) {
      const Step& st = p.steps[s];
      struct Pending { u32 dst; u32 v[NL]; };
      std::vector<Pending> pend;
      for (unsigned lane = 0; lane < 64; lane++) {
        unsigned inst = lane / p.W;
        if (inst >= p.G) continue;
        unsigned lane_in = lane - inst * p.W;
        // lane split: lane_in is the physical lane; a K_DOT lane-op is the sum of its sub-lanes' accumulators (computed when sub-lane 0 is visited),
        // every other kind runs on sub-lane 0 with the descriptor of its logical lane
        const unsigned S = p.lsplit, lg = lane_in / S, sub = lane_in % S;
        if (lg >= st.nlanes || sub != 0) continue;
        LaneCtx cx; cx.inst = p.inst_base(inst) - (p.shared_consts ? 2u : 0u); cx.shared = p.shared_consts; cx.item = blk * p.G + inst; cx.live = cx.item < n_items;
        Pending pd;
        u32 dw[8] = {0};
        const u32* gd = p.descs.data() + st.desc_off + (st.kind == K_DOT ? lane_in : lg) * st.stride;
        memcpy(dw, gd, (st.stride < 8 ? st.stride : 8) * 4);
        if (st.kind == K_DOT) {
          u64 acc[2 * NL];
          dot_init(acc, st, dw[0]);
          for (u32 r = 0; r < st.p0; r++) { const u32* rd = gd + DOT_HDR_WORDS + DOT_ROUND_WORDS * r; dot_round(acc, round_shape(st, r), round_signs(gd[1], r), rd[0], rd[1], rd[2], rd[3], lds, cx); }
          for (unsigned j = 1; j < S; j++) {   // the other sub-lanes: their own descriptors, their own (bias-free) accumulators
            const u32* gj = gd + j * st.stride;
            u64 aj[2 * NL];
            dot_init(aj, st, gj[0]);
            for (u32 r = 0; r < st.p0; r++) { const u32* rd = gj + DOT_HDR_WORDS + DOT_ROUND_WORDS * r; dot_round(aj, round_shape(st, r), round_signs(gj[1], r), rd[0], rd[1], rd[2], rd[3], lds, cx); }
            for (int c = 0; c < 2 * NL; c++) acc[c] += aj[c];
          }
          pd.dst = dot_finish(pd.v, acc, st, dw, lds, cx, qp_table);
        } else pd.dst = exec_lane(st, dw, lds, cx, bufs, pd.v, qp_table);
        if (pd.dst != 0xffffffffu) pend.push_back(pd);
      }
      for (auto& pd : pend) st14(lds, pd.dst, pd.v);
    }
  }
}

// ---- translated programs (aot.h) on the host: the step bodies of the ahead-of-time kernels (aot_exec.h), every lane's results committed after all lanes of the
// step have read their operands (on the device the LDS operations of a wavefront execute in order)
struct HostDesc {
  const u32* blk; u32 lane;   // blk: word 0 of lane 0
  V4 quad(u32 i) const { const u32* q = blk + ((size_t)i * 64 + lane) * 4; return V4{q[0], q[1], q[2], q[3]}; }
};
struct Pend { u32 dst; u32 v[NL]; };
#define SIM_CASE(ID, KIND, P0, FLAGS, T, SH0, SH1, CNT) \
  case ID: aot_step<KIND, P0, FLAGS, T, SH0, SH1>(d, lds, item, live, bufs, qp, [&](u32 dst, const u32* res) { Pend pd; pd.dst = dst; memcpy(pd.v, res, NL * 4); pend.push_back(pd); }); break;
#define SIM_TABLE(PART, NAME, Q0, Q1, Q2, Q3, Q4)                                                                                                     \
  static const AotSig sim_sigs_##NAME[] = {AOT_SIGS_##NAME(SIM_ROW)};                                                                      \
  static void sim_step_##NAME(u32 sig, const HostDesc& d, char* lds, u32 item, bool live, const IOBuf* bufs, const u32* qp, std::vector<Pend>& pend) { \
    switch (sig) { AOT_SIGS_##NAME(SIM_CASE) default: abort(); }                                                                          \
  }
#define SIM_ROW(ID, KIND, P0, FLAGS, T, SH0, SH1, CNT) {KIND, P0, FLAGS, T, SH0, SH1},
NBLS_AOT_KERNELS(SIM_TABLE)
#define SIM_TABLE_EXTRA(PART, NAME, E0, E1) SIM_TABLE(PART, NAME, E0, E1, E0, E1, E0)
NBLS_AOT_EXTRA_KERNELS(SIM_TABLE_EXTRA)   // the kernels of the programs outside ProgId (programs.h ExtraProg)
// lane-split kernels (aot.h NBLS_AOT_LS_KERNELS): the same bodies with LS = 4.  The device sums the columns of the four sub-lanes of a lane-op with two DPP stages
// (lane i <- v[i] + v[i+1] + v[i+2] + v[i+3] inside rows of 16 lanes); here the lanes of a step are visited from 63 down to 0, every lane leaves its columns in
// g_ls_cols before it takes the sum, so the three partners of a sub-lane 0 are already there.
static u64 g_ls_cols[64][2 * NL];
static unsigned g_ls_lane = 0, g_ls_width = 4;
static void sim_ls_sum(u64* acc, int nc) {
  const unsigned i = g_ls_lane;
  memcpy(g_ls_cols[i], acc, (size_t)nc * sizeof(u64));
  for (unsigned k = 1; k < g_ls_width; k++) if (i + k < 64 && (i + k) / 16 == i / 16) for (int c = 0; c < nc; c++) acc[c] += g_ls_cols[i + k][c];
}
#undef SIM_CASE
#define SIM_CASE(ID, KIND, P0, FLAGS, T, SH0, SH1, CNT) \
  case ID: aot_step<KIND, P0, FLAGS, T, SH0, SH1, 4>(d, lds, item, live, bufs, qp, [&](u32 dst, const u32* res) { Pend pd; pd.dst = dst; memcpy(pd.v, res, NL * 4); pend.push_back(pd); }); break;
NBLS_AOT_LS_KERNELS(SIM_TABLE)
#undef SIM_CASE
#define SIM_CASE(ID, KIND, P0, FLAGS, T, SH0, SH1, CNT) \
  case ID: aot_step<KIND, P0, FLAGS, T, SH0, SH1, 2>(d, lds, item, live, bufs, qp, [&](u32 dst, const u32* res) { Pend pd; pd.dst = dst; memcpy(pd.v, res, NL * 4); pend.push_back(pd); }); break;
NBLS_AOT_LS2_KERNELS(SIM_TABLE)
typedef void (*SimStepFn)(u32, const HostDesc&, char*, u32, bool, const IOBuf*, const u32*, std::vector<Pend>&);
struct SimKernel { int prog_id[5]; SimStepFn fn; const AotSig* sigs; unsigned nsigs; unsigned ls; };   // ls: sub-lanes per lane-op (0: none)
#define SIM_ENTRY(PART, NAME, Q0, Q1, Q2, Q3, Q4) {{(int)Q0, (int)Q1, (int)Q2, (int)Q3, (int)Q4}, sim_step_##NAME, sim_sigs_##NAME, (unsigned)(sizeof(sim_sigs_##NAME) / sizeof(AotSig)), 0},
#define SIM_ENTRY_LS(PART, NAME, Q0, Q1, Q2, Q3, Q4) {{(int)Q0, (int)Q1, (int)Q2, (int)Q3, (int)Q4}, sim_step_##NAME, sim_sigs_##NAME, (unsigned)(sizeof(sim_sigs_##NAME) / sizeof(AotSig)), 4},
#define SIM_ENTRY_LS2(PART, NAME, Q0, Q1, Q2, Q3, Q4) {{(int)Q0, (int)Q1, (int)Q2, (int)Q3, (int)Q4}, sim_step_##NAME, sim_sigs_##NAME, (unsigned)(sizeof(sim_sigs_##NAME) / sizeof(AotSig)), 2},
// an ExtraProg is entered as P_COUNT + 1 + its number, as in aot_kernel.hip
#define SIM_XP(E) ((int)E == (int)XP_COUNT ? (int)P_COUNT : (int)P_COUNT + 1 + (int)E)
#define SIM_ENTRY_EXTRA(PART, NAME, E0, E1) {{SIM_XP(E0), SIM_XP(E1), (int)P_COUNT, (int)P_COUNT, (int)P_COUNT}, sim_step_##NAME, sim_sigs_##NAME, (unsigned)(sizeof(sim_sigs_##NAME) / sizeof(AotSig)), 0},
static const SimKernel g_sim_kernels[] = {NBLS_AOT_KERNELS(SIM_ENTRY) NBLS_AOT_LS_KERNELS(SIM_ENTRY_LS) NBLS_AOT_LS2_KERNELS(SIM_ENTRY_LS2) NBLS_AOT_EXTRA_KERNELS(SIM_ENTRY_EXTRA)};
static int g_sim_aot = 0;
// 0: ran; -2: the program has no ahead-of-time kernel; -3: its signatures are not in the kernel's table
// key: a ProgId, or P_COUNT + 1 + an ExtraProg; placed = false: the LDS slots as compiled, whatever row aot_layout.inc has for the program
static int sim_run_aot_program(int key, const Program& p, unsigned n_items, const IOBuf* bufs, bool placed = true) {
  const SimKernel* K = nullptr;
  if (key >= 0 && key != (int)P_COUNT) for (auto& k : g_sim_kernels) for (int j = 0; j < 5; j++) if (k.prog_id[j] == key) K = &k;
  if (!K) return -2;
  AotProgram ap;
  if (!(placed ? aot_translate(p, ap) : aot_translate_with(p, ap, nullptr)).empty()) return -3;
  std::vector<unsigned> map(ap.sigs.size());
  for (size_t i = 0; i < ap.sigs.size(); i++) { unsigned id = 0; while (id < K->nsigs && !(K->sigs[id] == ap.sigs[i])) id++; if (id == K->nsigs) return -3; map[i] = id; }
  const u32* qp_table = qp_table_words();
  std::vector<V4> lds4((size_t)ap.lds_bytes / 16 + 1);
  char* lds = (char*)lds4.data();
  const unsigned blocks = (n_items + p.G - 1) / p.G;
  for (unsigned blk = 0; blk < blocks; blk++) {
    memset(lds, 0xde, (size_t)ap.lds_bytes);
    for (unsigned g = 0; g < (p.shared_consts ? 1u : p.G); g++) for (unsigned c = 0; c < p.nconst; c++) memcpy(lds + g * p.inst_bytes() + c * p.slot_bytes, p.consts.data() + c * RAW_WORDS, NL * 4);
    for (size_t s = 0; s < ap.steps.size(); s++) {
      std::vector<Pend> pend;
      aot_sim_ls_hook() = K->ls ? sim_ls_sum : nullptr; g_ls_width = K->ls ? K->ls : 4;
      for (unsigned v = 0; v < 64; v++) {
        const unsigned lane = K->ls ? 63 - v : v;      // lane-split kernels: from the top down (sim_ls_sum)
        const unsigned inst = lane / p.W, item = blk * p.G + inst;
        HostDesc d; d.blk = ap.descs.data() + (size_t)ap.steps[s].y * 4; d.lane = lane;
        g_ls_lane = lane;
        K->fn(map[ap.steps[s].x & 0xffu], d, lds, item, inst < p.G && item < n_items, bufs, qp_table, pend);
      }
      for (auto& pd : pend) st14(lds, pd.dst, pd.v);
    }
  }
  return 0;
}
static int sim_run_aot(int prog, unsigned n_items, const IOBuf* bufs) {
  if (prog < 0 || prog >= (int)P_COUNT) return -2;
  return sim_run_aot_program(prog, get_program((ProgId)prog), n_items, bufs);
}

// The one-limb-per-lane form (pow_wide.h) on the host: a value of type U is the array of the 32 lanes of a wavefront's first two rows, every cross-lane move a loop.  The
// arithmetic the device does in 32 / 64 bits is checked here for what the device silently assumes: no 64-bit column overflows, the low-word additions never carry.
static unsigned long g_wide_violations = 0;
struct WideHost {
  struct U { u32 v[32]; };
  struct W { u64 v[32]; };
  const u32* in; u32* out; bool fp2; U tab[POW_TAB];
  template <class F> static U map(F f) { U r; for (int k = 0; k < 32; k++) r.v[k] = f(k); return r; }
  U konst(const u32* t16) const { return map([&](int k) { return t16[k & 15]; }); }
  U sel(const U& a, const U& b) const { return map([&](int k) { return k >= 16 ? b.v[k] : a.v[k]; }); }
  U add(const U& a, const U& b) const { return map([&](int k) { if ((u64)a.v[k] + b.v[k] > 0xffffffffull) g_wide_violations++; return a.v[k] + b.v[k]; }); }
  U sub(const U& a, const U& b) const { return map([&](int k) { if (a.v[k] < b.v[k]) g_wide_violations++; return a.v[k] - b.v[k]; }); }
  U and_(const U& a, u32 m) const { return map([&](int k) { return a.v[k] & m; }); }
  U shr(const U& a, int s) const { return map([&](int k) { return a.v[k] >> s; }); }
  U mul_lo(const U& a, u32 c) const { return map([&](int k) { return a.v[k] * c; }); }
  U lo(const W& w) const { return map([&](int k) { return (u32)w.v[k]; }); }
  W zero() const { W w; for (int k = 0; k < 32; k++) w.v[k] = 0; return w; }
  W mad(const U& a, const U& b, const W& acc) const { W w; for (int k = 0; k < 32; k++) { const unsigned __int128 t = (unsigned __int128)acc.v[k] + (unsigned __int128)a.v[k] * b.v[k]; if (t >> 64) g_wide_violations++; w.v[k] = (u64)t; } return w; }
  W mad_s(const U& a, u32 s, const W& acc) const { W w; for (int k = 0; k < 32; k++) { const unsigned __int128 t = (unsigned __int128)acc.v[k] + (unsigned __int128)a.v[k] * s; if (t >> 64) g_wide_violations++; w.v[k] = (u64)t; } return w; }
  W shr28(const W& a) const { W w; for (int k = 0; k < 32; k++) w.v[k] = a.v[k] >> 28; return w; }
  W add_lo(const W& a, const U& x) const { W w; for (int k = 0; k < 32; k++) { if ((a.v[k] >> 32) || (a.v[k] + x.v[k]) >> 32) g_wide_violations++; w.v[k] = (a.v[k] & 0xffffffff00000000ull) | (u32)((u32)a.v[k] + x.v[k]); } return w; }
  U bcast(const U& a, int i) const { return map([&](int k) { return a.v[(k & 16) | i]; }); }
  U xchg(const U& a) const { return map([&](int k) { return a.v[k ^ 16]; }); }
  U shl1(const U& a) const { return map([&](int k) { return (k & 15) == 15 ? 0u : a.v[k + 1]; }); }
  U shr1(const U& a) const { return map([&](int k) { return (k & 15) == 0 ? 0u : a.v[k - 1]; }); }
  u32 lane_of(const U& a, int k) const { return a.v[k]; }
  U load() const { return map([&](int k) { return (k & 15) < NL && (fp2 || k < 16) ? in[k] : 0u; }); }      // in: the element's 16 (Fp) or 32 (Fp2) words
  void store(const U& a) { for (int k = 0; k < (fp2 ? 32 : 16); k++) out[k] = (k & 15) < NL ? a.v[k] : 0u; }
  void tab_put(int e, const U& a) { tab[e] = a; }
  U tab_get(int e) const { return tab[e]; }
};
// ---- the one-limb-per-lane interpreter (wide_exec.h, vm_wide_kernel.hip) on the host: a value is the array of a row's sixteen lanes; every lane-op of a step reads,
// then all results are committed (the device's two barriers).  The 32 / 64-bit assumptions of the device code are checked: g_wide_violations counts them.
struct WideRowHost {
  struct I { i32 v[16]; };
  struct W { i64 v[16]; };
  const char* lds; u32 base;
  u32 addr(u32 f) const { return (f & 2u) ? base + f - 2u : f; }
  template <class F> static I map(F f) { I r; for (int k = 0; k < 16; k++) r.v[k] = f(k); return r; }
  static i32 chk32(i64 x) { if (x > 0x7fffffffll || x < -0x80000000ll) { g_wide_violations++; if (getenv("NBLS_SIM_WIDE_DEBUG")) fprintf(stderr, "wide: 32-bit overflow %lld\n", (long long)x); } return (i32)x; }
  I zero() const { return map([](int) { return 0; }); }
  void fence() const {}
  bool skip_rows() const { return false; }
  I konst(u32 c) const { return map([&](int) { return (i32)c; }); }
  I add(const I& a, const I& b) const { return map([&](int k) { return chk32((i64)a.v[k] + b.v[k]); }); }
  I sub(const I& a, const I& b) const { return map([&](int k) { return chk32((i64)a.v[k] - b.v[k]); }); }
  I and_(const I& a, u32 m) const { return map([&](int k) { return (i32)((u32)a.v[k] & m); }); }
  I low13(const I& a) const { return map([&](int k) { return k < 13 ? (i32)((u32)a.v[k] & LMASK) : a.v[k]; }); }
  I carry13(const I& a) const { return map([&](int k) { return k < 13 ? a.v[k] : 0; }); }
  I sar(const I& a, int s) const { return map([&](int k) { return a.v[k] >> s; }); }
  I mul_lo(const I& a, u32 c) const { return map([&](int k) { return (i32)((u32)a.v[k] * c); }); }
  I mul_small(const I& a, u32 c) const { return map([&](int k) { return chk32((i64)a.v[k] * (i64)c); }); }
  I muls(const I& a, int c) const { return map([&](int k) { return chk32((i64)a.v[k] * (i64)c); }); }
  // fp_inv_wide.h
  I or_(const I& a, const I& b) const { return map([&](int k) { return a.v[k] | b.v[k]; }); }
  I spread(i32 s) const { return map([&](int) { return s; }); }
  i32 first(const I& a) const { for (int k = 1; k < 16; k++) if (a.v[k] != a.v[0]) g_wide_violations++; return a.v[0]; }      // (must be row-uniform)
  I plimbs() const { const u32 P[NL] = NBLS_P28; return map([&](int k) { return k < NL ? (i32)P[k] : 0; }); }
  u32 nonzero_mask(const I& a) const { u32 m = 0; for (int k = 0; k < 16; k++) if (a.v[k] != 0) m |= 1u << k; return m; }
  I gather(const I& a, u32 j) const { return map([&](int) { return a.v[j & 15u]; }); }
  I pick(u32 lanebit, const I& a, const I& b) const { return map([&](int k) { return ((lanebit >> k) & 1u) ? a.v[k] : b.v[k]; }); }
  I lane_eq(u32 j, const I& a, const I& b) const { return map([&](int k) { return (u32)k == j ? a.v[k] : b.v[k]; }); }
  I lo(const W& w) const { return map([&](int k) { return (i32)w.v[k]; }); }
  W wzero() const { W w; for (int k = 0; k < 16; k++) w.v[k] = 0; return w; }
  static i64 chk64(__int128 t) { if (t > (__int128)0x7fffffffffffffffll || t < -(__int128)0x7fffffffffffffffll - 1) { g_wide_violations++; if (getenv("NBLS_SIM_WIDE_DEBUG")) fprintf(stderr, "wide: 64-bit overflow\n"); } return (i64)t; }
  W mad(const I& a, const I& b, const W& acc) const { W w; for (int k = 0; k < 16; k++) w.v[k] = chk64((__int128)acc.v[k] + (__int128)a.v[k] * b.v[k]); return w; }
  W mad_p(const I& ml, const W& acc) const { const u32 P[NL] = NBLS_P28; W w; for (int k = 0; k < 16; k++) w.v[k] = chk64((__int128)acc.v[k] + (__int128)(k < NL ? P[k] : 0u) * ml.v[0]); return w; }
  W mad_pq(const I& q, const W& acc) const { const u32 P[NL] = NBLS_P28; W w; for (int k = 0; k < 16; k++) w.v[k] = chk64((__int128)acc.v[k] + (__int128)(k < NL ? P[k] : 0u) * q.v[k]); return w; }
  W sar28(const W& a) const { W w; for (int k = 0; k < 16; k++) w.v[k] = a.v[k] >> 28; return w; }
  W addw(const W& a, const I& x) const { W w; for (int k = 0; k < 16; k++) w.v[k] = chk64((__int128)a.v[k] + x.v[k]); return w; }
  W addww(const W& a, const W& b) const { W w; for (int k = 0; k < 16; k++) w.v[k] = chk64((__int128)a.v[k] + b.v[k]); return w; }
  I wred_q(const I& top) const { return map([&](int k) { i32 t = top.v[k] - 9; t = t < 0 ? 0 : t; const u32 q = (u32)(((u64)(u32)t * 2642610142u) >> 48); return (i32)(q > (u32)(QP_TABLE_ENTRIES - 1) ? (u32)(QP_TABLE_ENTRIES - 1) : q); }); }
  I bcast(const I& a, int i) const { return map([&](int) { return a.v[i]; }); }
  I shl1(const I& a) const { return map([&](int k) { return k == 15 ? 0 : a.v[k + 1]; }); }
  I shr1(const I& a) const { return map([&](int k) { return k == 0 ? 0 : a.v[k - 1]; }); }
  I ld(u32 f) const { const u32 off = addr(f); return map([&](int k) { i32 x; memcpy(&x, lds + off + 4 * k, 4); return x; }); }
  I gload(const u32* g, bool live) const { return map([&](int k) { return (live && k < NL) ? (i32)g[k] : 0; }); }
  void gstore(u32* g, const I& v, bool live) const { if (live) for (int k = 0; k < 16; k++) g[k] = (u32)v.v[k]; }
};
struct WideDescHost { const u32* w; u32 operator()(int k) const { return w[k]; } };
// 0: ran; -4: the program has a step the form does not implement (or shared constants / a lane split)
static int sim_run_wide(const Program& p, unsigned n_items, const IOBuf* bufs) {
  if (p.lsplit != 1 || p.W > 16) return -4;
  for (auto& st : p.steps) if (!wide_step_supported(st, p.descs.data())) return -4;
  const u32 base = p.inst_base(0);
  std::vector<u32> image((size_t)(base + p.inst_bytes()) / 4 + 8);
  char* lds = (char*)image.data();
  for (unsigned item = 0; item < n_items; item++) {
    std::fill(image.begin(), image.end(), 0u);
    for (unsigned c = 0; c < p.nconst; c++) memcpy(lds + c * p.slot_bytes, p.consts.data() + c * RAW_WORDS, NL * 4);
    for (auto& st : p.steps) {
      struct Pending { u32 dst; WideRowHost::I v; };
      std::vector<Pending> pend;
      for (unsigned row = 0; row < st.nlanes; row++) {
        WideRowHost l; l.lds = lds; l.base = base;
        WideOps<WideRowHost> o(l);
        WideDescHost d{p.descs.data() + st.desc_off + row * st.stride};
        Pending pd;
        if (wide_step(o, st, d, bufs, item, true, pd.dst, pd.v)) pend.push_back(pd);
      }
      for (auto& pd : pend) { const u32 a = (pd.dst & 2u) ? base + pd.dst - 2u : pd.dst; memcpy(lds + a, pd.v.v, 64); }
    }
  }
  return 0;
}
// g1_wide.h on the host: the rows of a round one after the other, their results written once all of them have read (the device: one wavefront, LDS in program order)
static const u32 GW_TABLE_HOST[GW_TABLE_WORDS] = GW_TABLE_INIT;
static void sim_g1_wide_combine(const u32* S, int nwin, int shift, u32* out) {
  std::vector<u32> image((size_t)GW_SLOTS * 16, 0u);
  char* lds = (char*)image.data();
  auto fetch = [&](const u32* pt, int s0, int s1, int s2) { const int sl[3] = {s0, s1, s2}; for (int r = 0; r < 3; r++) { memset(lds + sl[r] * 64, 0, 64); memcpy(lds + sl[r] * 64, pt + r * RAW_WORDS, NL * 4); } };
  auto run_round = [&](int q, int p0) {
    WideRowHost::I res[4];
    for (int row = 0; row < 4; row++) {
      WideRowHost l; l.lds = lds; l.base = 0;
      WideOps<WideRowHost> o(l); WideG1<WideRowHost> g(o);
      const u32* d = GW_TABLE_HOST + (4 * q + row) * GW_ROW_WORDS;
      res[row] = p0 == 1 ? g.round<1>(d) : g.round<2>(d);
    }
    for (int row = 0; row < 4; row++) memcpy(lds + GW_TABLE_HOST[(4 * q + row) * GW_ROW_WORDS + 4] * 64, res[row].v, 64);
  };
  fetch(S + (size_t)(nwin - 1) * 3 * RAW_WORDS, GW_X, GW_U, GW_Z);
  for (int w = nwin - 2; w >= 0; w--) {
    fetch(S + (size_t)w * 3 * RAW_WORDS, GW_X2, GW_Y2, GW_Z2);
    for (int i = 0; i < shift; i++) { run_round(0, 1); run_round(1, 1); }
    for (int q = 0; q < GW_ADD_ROUNDS; q++) run_round(GW_DBL_ROUNDS + q, 2);
  }
  for (int row = 0; row < 3; row++) {
    WideRowHost l; l.lds = lds; l.base = 0;
    WideOps<WideRowHost> o(l); WideG1<WideRowHost> g(o);
    const WideRowHost::I v = row == 0 ? l.ld(GW_X * 64u) : row == 1 ? l.sub(l.ld(GW_U * 64u), l.ld(GW_V * 64u)) : l.ld(GW_Z * 64u);
    const WideRowHost::I e = g.leave(v, row == 1 ? 2u : 1u);
    for (int k = 0; k < 16; k++) { if (e.v[k] < 0 || (k < NL - 1 && e.v[k] > (i32)LMASK)) g_wide_violations++; out[row * RAW_WORDS + k] = (u32)e.v[k]; }
  }
}
static int g_sim_wide = 0;
// fr_workgroup.h on the host
static bool g_lanes_down = false;
template <uint32_t LANES> static FrWorkgroup<LANES> sim_wg() { return FrWorkgroup<LANES>{g_lanes_down}; }
// the table of roots as kzg_roots_kernel builds it, and kzg_inv_roots_kernel's permutation of it
static std::vector<Fr> sim_roots(unsigned log2_n) {
  std::vector<Fr> t((size_t)1 << log2_n);
  const Fr omega = fr_omega(log2_n);
  for (u32 j = 0; j < t.size(); j++) t[j] = fr_root_entry(omega, log2_n, j);
  return t;
}
static std::vector<Fr> sim_inv_roots(unsigned log2_n, const std::vector<Fr>& roots) {
  std::vector<Fr> t(roots.size());
  for (u32 j = 0; j < t.size(); j++) t[j] = roots[fr_inv_root_index(log2_n, j)];
  return t;
}
// n polynomials through kzg_ntt_kernel's body, one workgroup each (the arrays as nbls_kzg_ntt_launch takes them)
static void sim_ntt(unsigned log2_n, unsigned mode, size_t n, const uint8_t* in32, const uint8_t* shift32, size_t shift_stride, uint8_t* out32, uint8_t* coef32, int8_t* status) {
  const std::vector<Fr> roots = sim_roots(log2_n), iroots = sim_inv_roots(log2_n, roots);
  const size_t row = (size_t)32 << log2_n, out_stride = mode == FR_NTT_CELLS ? 2 * row : row;
  std::vector<u32> a(row / 4);
  Fr s = fr_one(); u32 bad = 0, zero = 0;
  for (size_t p = 0; p < n; p++)
    kzg_ntt_body(sim_wg<FR_NTT_LANES>(), log2_n, mode, in32 + row * p, shift32 ? shift32 + shift_stride * p : nullptr, roots.data(), iroots.data(), out32 + out_stride * p, out_stride,
                 coef32 ? coef32 + row * p : nullptr, status ? status + p : nullptr, a.data(), &s, &bad, &zero);
}
// slot placement of a program's translated form (aot_layout.h): out = {has a valid table row, LDS read cycles per wavefront as compiled, with the placement, without any conflict}
static int sim_layout_info(const Program& p, unsigned long* out4) {
  const AotLayout* l = aot_layout_for(p);
  const AotLdsCost c0 = aot_layout_cost(p, AotLayout());
  const AotLdsCost c1 = l ? aot_layout_cost(p, *l) : c0;
  out4[0] = l ? 1 : 0; out4[1] = c0.cycles; out4[2] = c1.cycles; out4[3] = c0.floor;
  return 0;
}
extern "C" {
// the one-limb-per-lane form for the programs it implements (others run as usual): 0 off, 1 on; nbls_sim_wide_violations: device assumptions violated since the last call (0 on a correct build)
__attribute__((visibility("default"))) void nbls_sim_set_wide(int on) { g_sim_wide = on; }
// the window combination of the G1 MSM with one limb per lane (g1_wide.h): S = nwin projective points of 3 raw elements, out = sum_w 2^(shift w) S_w (3 raw elements)
__attribute__((visibility("default"))) void nbls_sim_g1_wide_combine(const u32* S, int nwin, int shift, u32* out) { sim_g1_wide_combine(S, nwin, shift, out); }
__attribute__((visibility("default"))) unsigned long nbls_sim_wide_violations() { const unsigned long v = g_wide_violations; g_wide_violations = 0; return v; }
__attribute__((visibility("default"))) int nbls_sim_wide_supported(int prog) { if (prog < 0 || prog >= (int)P_COUNT) return 0; const Program& p = get_program((ProgId)prog); if (p.lsplit != 1 || p.W > 16) return 0; for (auto& st : p.steps) if (!wide_step_supported(st, p.descs.data())) return 0; return 1; }
// translated programs (aot.h) instead of the interpreter's semantics for the programs that have an ahead-of-time kernel: 0 off, 1 on
__attribute__((visibility("default"))) void nbls_sim_set_aot(int on) { g_sim_aot = on; }
__attribute__((visibility("default"))) int nbls_sim_has_aot(int prog) { if (prog < 0 || prog >= (int)P_COUNT) return 0; for (auto& k : g_sim_kernels) for (int j = 0; j < 5; j++) if (k.prog_id[j] == prog) return 1; return 0; }
// bufs: 8 pointers + 8 strides
__attribute__((visibility("default"))) int nbls_sim_run(int prog, unsigned n_items, uint8_t** ptrs, const uint64_t* strides) {
  if (prog < 0 || prog >= P_COUNT) return -1;
  IOBuf b[MAX_BUFS];
  for (int i = 0; i < MAX_BUFS; i++) { b[i].ptr = ptrs[i]; b[i].stride = strides[i]; }
  if (g_sim_wide) { const int r = sim_run_wide(get_program((ProgId)prog), n_items, b); if (r != -4) return r; }
  if (g_sim_aot) { const int r = sim_run_aot(prog, n_items, b); if (r != -2) return r; }
  sim_run(get_program((ProgId)prog), n_items, b);
  return 0;
}
// The programs outside ProgId (programs.h ExtraProg; nbls_sim_run refuses everything from P_COUNT on): count, name, the static verifier (0 = passed; the message goes to
// stderr), and a run -- aot = 0: the interpreter's semantics; 1: the translated form on the step bodies of the program's ahead-of-time kernel (-2: it has none, -3: its
// signatures are not in the kernel's table); 2: the same with the LDS slots as compiled, the form a program takes while aot_layout.inc has no current row for it
__attribute__((visibility("default"))) int nbls_sim_extra_count(void) { return XP_NUMBERED; }
__attribute__((visibility("default"))) const char* nbls_sim_extra_name(int xp) { return xp >= 0 && xp < XP_NUMBERED ? get_extra_program((ExtraProg)xp).name.c_str() : nullptr; }
static int sim_extra_verify(int xp) {
  const std::string e = verify_program(get_extra_program((ExtraProg)xp));
  if (!e.empty()) fprintf(stderr, "nbls_sim_extra_verify: %s\n", e.c_str());
  return e.empty() ? 0 : 1;
}
static int sim_extra_run(int xp, int aot, unsigned n_items, uint8_t** ptrs, const uint64_t* strides) {
  IOBuf b[MAX_BUFS];
  for (int i = 0; i < MAX_BUFS; i++) { b[i].ptr = ptrs[i]; b[i].stride = strides[i]; }
  const Program& p = get_extra_program((ExtraProg)xp);
  if (aot) return sim_run_aot_program((int)P_COUNT + 1 + xp, p, n_items, b, aot != 2);
  sim_run(p, n_items, b);
  return 0;
}
__attribute__((visibility("default"))) int nbls_sim_extra_verify(int xp) { return xp < 0 || xp >= XP_NUMBERED ? -1 : sim_extra_verify(xp); }
__attribute__((visibility("default"))) int nbls_sim_extra_run(int xp, int aot, unsigned n_items, uint8_t** ptrs, const uint64_t* strides) {
  return xp < 0 || xp >= XP_NUMBERED ? -1 : sim_extra_run(xp, aot, n_items, ptrs, strides);
}
// The same by name, for every program of ExtraProg -- the numbered entry points above stop at XP_NUMBERED (programs.h); -1 for a name that is none
static int sim_extra_by_name(const char* name) {
  if (name) for (int i = 0; i < (int)XP_COUNT; i++) if (get_extra_program((ExtraProg)i).name == name) return i;
  return -1;
}
__attribute__((visibility("default"))) int nbls_sim_extra_verify_named(const char* name) { const int xp = sim_extra_by_name(name); return xp < 0 ? -1 : sim_extra_verify(xp); }
__attribute__((visibility("default"))) int nbls_sim_extra_run_named(const char* name, int aot, unsigned n_items, uint8_t** ptrs, const uint64_t* strides) {
  const int xp = sim_extra_by_name(name);
  return xp < 0 ? -1 : sim_extra_run(xp, aot, n_items, ptrs, strides);
}
// the line nbls_sim_stats prints per numbered program, for one of these; -1 for a name that is none
__attribute__((visibility("default"))) int nbls_sim_extra_stats_named(const char* name) { const int xp = sim_extra_by_name(name); if (xp < 0) return -1; print_stats(get_extra_program((ExtraProg)xp)); return 0; }
// lanes per item of a numbered program as it compiled in this process (which form of a program an environment switch selected)
__attribute__((visibility("default"))) int nbls_sim_program_lanes(int prog) { return prog < 0 || prog >= P_COUNT ? -1 : (int)get_program((ProgId)prog).W; }
// what pairing_core (pipelines_pairing.cpp) asks before it picks the line program of a call with final exponentiation
__attribute__((visibility("default"))) int nbls_sim_lines_fe_enabled(void) { return lines_fe_enabled() ? 1 : 0; }
// nbls_sim_layout_info for one of these
__attribute__((visibility("default"))) int nbls_sim_extra_layout_info_named(const char* name, unsigned long* out4) {
  const int xp = sim_extra_by_name(name); if (xp < 0) return -1;
  return sim_layout_info(get_extra_program((ExtraProg)xp), out4);
}
// out = in^-1 on raw elements (16 words each): the same fp_mont_inverse routine the inversion kernel runs per lane
// the same inverse with one limb per lane (fp_inv_wide.h), one element after the other
__attribute__((visibility("default"))) void nbls_sim_fp_inv_wide(unsigned n, const u32* in, u32* out) {
  const u32 R3[NL] = NBLS_R3_INIT;
  for (unsigned e = 0; e < n; e++) {
    WideRowHost l; l.lds = nullptr; l.base = 0;
    WideOps<WideRowHost> o(l); WideInv<WideRowHost> w(o);
    WideRowHost::I y, r3;
    for (int k = 0; k < 16; k++) { y.v[k] = k < NL ? (i32)in[SLOT_WORDS * e + k] : 0; r3.v[k] = k < NL ? (i32)R3[k] : 0; }
    const WideRowHost::I r = w.invert(y, r3);
    for (int k = 0; k < 16; k++) { if (k < NL && (r.v[k] < 0 || (k < NL - 1 && r.v[k] > (i32)LMASK))) g_wide_violations++; out[SLOT_WORDS * e + k] = k < NL ? (u32)r.v[k] : 0u; }
  }
}
__attribute__((visibility("default"))) void nbls_sim_fp_inv(unsigned n, const u32* in, u32* out) {
  for (unsigned k = 0; k < n; k++) { u32 r[NL]; fp_mont_inverse(r, in + SLOT_WORDS * k); memcpy(out + SLOT_WORDS * k, r, NL * 4); out[SLOT_WORDS * k + 14] = out[SLOT_WORDS * k + 15] = 0; }
}
// out = in^e; which: 0 = (p+1)/4 on Fp, 1 = (p^2+7)/16 on Fp2, 2 = (p^2-9)/16 on Fp2, 3 = (p-3)/4 on Fp (stand-ins for the pow kernels; raw elements of 16 words)
static void mmh(u32* r, const u32* a, const u32* b) { u32 t[NL]; mont_mul28(t, a, b); memcpy(r, t, NL * 4); }
static void addh(u32* r, const u32* a, const u32* b) { u32 t[NL]; for (int i = 0; i < NL; i++) t[i] = a[i] + b[i]; carry_norm(t); memcpy(r, t, NL * 4); }
static void subh(u32* r, const u32* a, const u32* b) { const u32 BIAS[NL] = NBLS_BIAS16_28; u32 t[NL]; for (int i = 0; i < NL; i++) t[i] = a[i] + BIAS[i] - b[i]; carry_norm(t); memcpy(r, t, NL * 4); }
static void fp2mulh(u32* r, const u32* a, const u32* b) {   // elements: c0 at [0..13], c1 at [16..29]
  u32 t1[NL], t2[NL], s1[NL], s2[NL], m[NL];
  mmh(t1, a, b); mmh(t2, a + 16, b + 16); addh(s1, a, a + 16); addh(s2, b, b + 16); mmh(m, s1, s2);
  u32 r0[NL], r1[NL], u[NL]; subh(r0, t1, t2); addh(u, t1, t2); subh(r1, m, u);
  u32 one[NL]; memcpy(one, NBLS_R1, NL * 4); mmh(r0, r0, one); mmh(r1, r1, one);   // contract (keeps values far below the 16p subtraction bias)
  memset(r, 0, 32 * 4); memcpy(r, r0, NL * 4); memcpy(r + 16, r1, NL * 4);
}
// plain square-and-multiply (what nbls_sim_fp_pow was until round 5): kept as the independent check of the chains below
__attribute__((visibility("default"))) void nbls_sim_fp_pow_naive(unsigned n, const u32* in, u32* out, int which) {
  const uint64_t* e = which == 0 ? NBLS_EXP_P_PLUS_1_DIV_4 : which == 1 ? NBLS_EXP_P2_PLUS_7_DIV_16 : which == 2 ? NBLS_EXP_P2_MINUS_9_DIV_16 : NBLS_EXP_P_MINUS_3_DIV_4;
  int bits = which == 0 ? NBLS_P_PLUS_1_DIV_4_BITS : which == 1 ? NBLS_P2_PLUS_7_DIV_16_BITS : which == 2 ? NBLS_P2_MINUS_9_DIV_16_BITS : NBLS_P_MINUS_3_DIV_4_BITS;
  for (unsigned k = 0; k < n; k++) {
    if (which == 0 || which == 3) {
      u32 acc[16] = {0}; memcpy(acc, NBLS_R1, NL * 4);
      for (int i = bits - 1; i >= 0; i--) { mmh(acc, acc, acc); if ((e[i >> 6] >> (i & 63)) & 1) mmh(acc, acc, in + 16 * k); }
      memcpy(out + 16 * k, acc, 64);
    } else {
      u32 acc[32] = {0}; memcpy(acc, NBLS_R1, NL * 4);
      for (int i = bits - 1; i >= 0; i--) { fp2mulh(acc, acc, acc); if ((e[i >> 6] >> (i & 63)) & 1) fp2mulh(acc, acc, in + 32 * k); }
      memcpy(out + 32 * k, acc, 128);
    }
  }
}
// The chains of pow_exec.h on the host: the sequences (tables, sliding windows, the split of the Fp2 exponents) and the lane arithmetic the kernels of
// pow_kernels.hip run; a lane pair of the Fp2 kernel is one value with both components here.
struct FpHost {
  struct V { u32 v[NL]; };
  const u32* in; u32* out; u32 tab[POW_TAB][NL];
  void sqr(V& r, const V& a) { u32 t[NL]; mont_sqr28(t, a.v); memcpy(r.v, t, sizeof t); }
  void mul(V& r, const V& a, const V& b) { u32 t[NL]; mont_mul28(t, a.v, b.v); memcpy(r.v, t, sizeof t); }
  void copy(V& r, const V& a) { r = a; }
  void load(V& r) { memcpy(r.v, in, NL * 4); }
  void store(const V& a) { memset(out, 0, 64); memcpy(out, a.v, NL * 4); }
  void tab_put(int j, const V& a) { memcpy(tab[j], a.v, NL * 4); }
  void tab_get(V& r, unsigned j) { memcpy(r.v, tab[j], NL * 4); }
};
struct Fp2Host {
  struct V { u32 c[2][NL]; };
  const u32* in; u32* out; V tab[POW_TAB];
  void sqr(V& r, const V& a) { V t; fp2_sqr_c(t.c[0], a.c[0], a.c[1], false); fp2_sqr_c(t.c[1], a.c[1], a.c[0], true); r = t; }
  void mul(V& r, const V& a, const V& b) { V t; fp2_mul_c(t.c[0], a.c[0], a.c[1], b.c[0], b.c[1], false); fp2_mul_c(t.c[1], a.c[1], a.c[0], b.c[1], b.c[0], true); r = t; }
  void conj(V& r, const V& a) { const u32 BIAS[NL] = NBLS_BIAS16_28; V t = a; for (int k = 0; k < NL; k++) t.c[1][k] = BIAS[k] - a.c[1][k]; carry_norm(t.c[0]); carry_norm(t.c[1]); r = t; }
  void copy(V& r, const V& a) { r = a; }
  void load(V& r) { for (int h = 0; h < 2; h++) mont_mul28(r.c[h], in + 16 * h, NBLS_R1); }
  void store(const V& a) { memset(out, 0, 128); memcpy(out, a.c[0], NL * 4); memcpy(out + 16, a.c[1], NL * 4); }
  void tab_put(int j, const V& a) { tab[j] = a; }
  void tab_get(V& r, unsigned j) { r = tab[j]; }
};
// the op list of exponent `which` as the pow kernels walk it: the Fp2 exponents through their shared part ((p - 3) / 4 - 2) / 4 (pow_exec.h fp2_pow_seq has the split)
static std::vector<unsigned char> sim_pow_ops(int which) {
  if (which == 0) return pow_make_ops(NBLS_EXP_P_PLUS_1_DIV_4, NBLS_P_PLUS_1_DIV_4_BITS);
  if (which != 1 && which != 2) return pow_make_ops(NBLS_EXP_P_MINUS_3_DIV_4, NBLS_P_MINUS_3_DIV_4_BITS);
  uint64_t K[6]; for (int j = 0; j < 6; j++) K[j] = NBLS_EXP_P_MINUS_3_DIV_4[j];
  K[0] -= 2;
  for (int j = 0; j < 6; j++) K[j] = (K[j] >> 2) | (j < 5 ? K[j + 1] << 62 : 0);
  return pow_make_ops(K, 377);
}
// out = in^e through the kernels' chains; which: 0 = (p+1)/4 on Fp, 1 = (p^2+7)/16 on Fp2, 2 = (p^2-9)/16 on Fp2, 3 = (p-3)/4 on Fp (raw elements of 16 words)
__attribute__((visibility("default"))) void nbls_sim_fp_pow(unsigned n, const u32* in, u32* out, int which) {
  const std::vector<unsigned char> ops = sim_pow_ops(which);
  const int nops = (int)(ops.size() / 2);
  for (unsigned k = 0; k < n; k++) {
    if (which == 0 || which == 3) { FpHost o; o.in = in + 16 * k; o.out = out + 16 * k; fp_pow_seq(o, ops.data(), nops); }
    else { Fp2Host o; o.in = in + 32 * k; o.out = out + 32 * k; fp2_pow_seq(o, ops.data(), nops, which == 1 ? 8 : 7); }
  }
}
// out = in^e through the one-limb-per-lane chains (which as nbls_sim_fp_pow); returns the number of violated device assumptions (0 on a correct build)
__attribute__((visibility("default"))) unsigned long nbls_sim_fp_pow_wide(unsigned n, const u32* in, u32* out, int which) {
  const std::vector<unsigned char> ops = sim_pow_ops(which);
  const int nops = (int)(ops.size() / 2);
  const WideConsts consts = wide_consts();
  g_wide_violations = 0;
  for (unsigned k = 0; k < n; k++) {
    if (which == 0 || which == 3) { WideHost l; l.in = in + 16 * k; l.out = out + 16 * k; l.fp2 = false; WideField<WideHost, false> f(l, consts); fp_pow_seq(f, ops.data(), nops); }
    else { WideHost l; l.in = in + 32 * k; l.out = out + 32 * k; l.fp2 = true; WideField<WideHost, true> f(l, consts); fp2_pow_seq(f, ops.data(), nops, which == 1 ? 8 : 7); }
  }
  return g_wide_violations;
}
// op list statistics of an exponent (tests): squarings, multiplications
__attribute__((visibility("default"))) void nbls_sim_pow_ops(int which, unsigned* out2) {
  const std::vector<unsigned char> ops = sim_pow_ops(which);
  out2[0] = out2[1] = 0;
  for (size_t k = 0; k < ops.size() / 2; k++) { out2[0] += ops[2 * k]; if (k && ops[2 * k + 1] != 0xff) out2[1]++; }
}
// canonical representative of raw elements (tests compare results that may differ by multiples of p)
__attribute__((visibility("default"))) void nbls_sim_fp_canon(unsigned n, const u32* in, u32* out) {
  for (unsigned k = 0; k < n; k++) { u32 t[NL]; mont_mul28(t, in + 16 * k, NBLS_R1); csub_p(t); memset(out + 16 * k, 0, 64); memcpy(out + 16 * k, t, NL * 4); }
}
// static verification of a compiled program (trace.h verify_program): 0 = clean, else the first violation in msg
__attribute__((visibility("default"))) int nbls_sim_verify(int prog, char* msg, unsigned cap) {
  if (prog < 0 || prog >= P_COUNT) return -1;
  const std::string e = verify_program(get_program((ProgId)prog));
  if (msg && cap) { snprintf(msg, cap, "%s", e.c_str()); }
  return e.empty() ? 0 : 1;
}
// the verifier on a deliberately damaged copy of a program: descriptor word `word` (or, with step_field >= 0, a header field of step `word`) is
// XOR-ed with `flip`; returns 1 and the violation when the damage is caught
__attribute__((visibility("default"))) int nbls_sim_verify_damaged(int prog, unsigned word, unsigned flip, int step_field, char* msg, unsigned cap) {
  if (prog < 0 || prog >= P_COUNT) return -1;
  Program p = get_program((ProgId)prog);
  if (step_field < 0) { if (word >= p.descs.size()) return -1; p.descs[word] ^= flip; }
  else { if (word >= p.steps.size()) return -1; Step& st = p.steps[word]; if (step_field == 0) st.desc_off ^= flip; else if (step_field == 1) st.nlanes ^= (uint8_t)flip; else if (step_field == 2) st.p0 ^= (uint8_t)flip; else st.kind ^= (uint8_t)flip; }
  const std::string e = verify_program(p);
  if (msg && cap) snprintf(msg, cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}
// sim_layout_info of a numbered program
__attribute__((visibility("default"))) int nbls_sim_layout_info(int prog, unsigned long* out4) {
  if (prog < 0 || prog >= P_COUNT) return -1;
  return sim_layout_info(get_program((ProgId)prog), out4);
}
// the scalar side of the endomorphism splits as the device runs it (scalar_split.h): dims = 2 / 4: base-|z| digits; dims = 0: the sign-aligned recoding (4 x 32 bytes per scalar)
// the weights of nbls_verify_multiple as rlc_kernels.hip derives them (rlc_weights.h): r_i for the set index i, 32 bytes big-endian
__attribute__((visibility("default"))) void nbls_sim_rlc_weight(const uint8_t* seed32, uint64_t i, uint8_t* out32) { rlc_weight(seed32, i, out32); }
__attribute__((visibility("default"))) void nbls_sim_scalar_split(unsigned n, unsigned dims, const uint8_t* scalars, uint8_t* out) {
  for (unsigned i = 0; i < n; i++) { if (dims) scalar_decompose(scalars + 32ull * i, dims, out + 32ull * dims * i); else scalar_sac_recode(scalars + 32ull * i, out + 128ull * i); }
}
// the scalar field as fr_kernels.hip runs it (fr_exec.h).  nbls_sim_fr_consts: r | -r^-1 mod 2^32 | R^2 mod r | R mod r | r - 2 as 8 + 1 + 8 + 8 + 8 words
__attribute__((visibility("default"))) void nbls_sim_fr_consts(u32* out33) {
  const Fr r2 = fr_r2(), one = fr_one();
  for (int i = 0; i < FR_NL; i++) { out33[i] = fr_mod(i); out33[9 + i] = r2.l[i]; out33[17 + i] = one.l[i]; out33[25 + i] = fr_rm2(i); }
  out33[8] = fr_n0();
}
// fr_op_kernel for every element: 32-byte big-endian operands (b = NULL for unary operations) -> out32 and status (5 where INV / DIV meets 0 mod r)
__attribute__((visibility("default"))) void nbls_sim_fr_op(unsigned n, int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32, int8_t* status) {
  for (unsigned i = 0; i < n; i++) status[i] = (int8_t)fr_op_bytes(op, a32 + 32ull * i, b32 ? b32 + 32ull * i : a32 + 32ull * i, out32 + 32ull * i);
}
// the conversions of fr_exec.h: wire bytes -> Montgomery limbs (to_mont != 0: fr_to_mont_kernel) or back (as fr_lagrange_out_kernel and fr_op_bytes do)
__attribute__((visibility("default"))) void nbls_sim_fr_convert(unsigned n, int to_mont, const uint8_t* in, uint8_t* out) {
  for (unsigned i = 0; i < n; i++) { if (to_mont) ((Fr*)out)[i] = fr_from_bytes(in + 32ull * i); else fr_to_bytes(((const Fr*)in)[i], out + 32ull * i); }
}
// nbls_fr_lagrange_launch: the conversion, fr_lagrange_kernel workgroup by workgroup (64 lanes, the wavefront's identifier range staged in tiles of 64, lanes past n running
// along with the last share) and fr_lagrange_out_kernel.  off: ngroups + 1 relative offsets; status: one byte per group (20 = unusable identifiers)
__attribute__((visibility("default"))) void nbls_sim_fr_lagrange(unsigned n, unsigned ngroups, const u32* off, const uint8_t* ids32, uint8_t* out32, int8_t* status) {
  const u32 W = 64;
  std::vector<Fr> x(n), lambda(n);
  std::vector<u32> group_of(n), bad_group(ngroups, 0);
  for (unsigned i = 0; i < n; i++) x[i] = fr_from_bytes(ids32 + 32ull * i);
  for (u32 k0 = 0; k0 < n; k0 += W) {
    u32 kk[W], g[W]; std::vector<FrLagrange> s;
    for (u32 l = 0; l < W; l++) { kk[l] = k0 + l < n ? k0 + l : n - 1; g[l] = fr_group_of(off, ngroups, kk[l]); s.push_back(fr_lagrange_begin(x[kk[l]])); }
    const u32 rb = off[g[0]], re = off[g[W - 1] + 1];
    for (u32 t = rb; t < re; t += W) {
      Fr tile[W];
      for (u32 l = 0; l < W; l++) tile[l] = x[t + l < re ? t + l : re - 1];
      const u32 cnt = re - t < W ? re - t : W;
      for (u32 l = 0; l < W; l++) fr_lagrange_tile(s[l], tile, t, cnt, off[g[l]], off[g[l] + 1], kk[l]);
    }
    for (u32 l = 0; l < W && k0 + l < n; l++) {
      u32 bad;
      lambda[k0 + l] = fr_lagrange_finish(s[l], &bad);
      group_of[k0 + l] = g[l];
      if (bad) bad_group[g[l]] |= 1;
    }
  }
  for (unsigned k = 0; k < n; k++) fr_store_be(fr_select((u32)0 - (u32)(bad_group[group_of[k]] != 0), fr_zero(), fr_from_mont(lambda[k])), out32 + 32ull * k);
  for (unsigned j = 0; j < ngroups; j++) status[j] = bad_group[j] ? 20 : 0;
}
// ---- The workgroup kernels of kzg_kernels.hip and groth16_kernels.hip: their bodies are fr_workgroup.h's, the text the device compiles, on the host's workgroup view -- a
// phase is every lane of the workgroup in turn, from lane 0 up or (nbls_sim_set_lane_order) from the top down.  An entry point is the argument rules of the device call that
// need no context (-1 = NBLS_EINVAL), the tables, the kernel's shared memory as arrays of exactly its size, a loop over the workgroups and the body's call.
__attribute__((visibility("default"))) void nbls_sim_set_lane_order(int descending) { g_lanes_down = descending != 0; }
__attribute__((visibility("default"))) int nbls_sim_fr_eval_roots(unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out32, int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || (n && (!evals32 || !z32 || !out32)) || (n << log2_n) > ((size_t)1 << 24)) return -1;
  const u32 N = 1u << log2_n, W = FR_EVAL_LANES;
  const std::vector<Fr> roots = sim_roots(log2_n);
  std::vector<Fr> part(W);
  std::vector<u32> pre((size_t)((N + W - 1) / W) * FR_NL * W);
  u32 hit = 0, bad = 0; int8_t st;
  for (size_t p = 0; p < n; p++)
    kzg_eval_body(sim_wg<FR_EVAL_LANES>(), log2_n, evals32 + 32ull * N * p, z32 + 32ull * p, roots.data(), out32 + 32ull * p, status ? status + p : &st, pre.data(), part.data(), &hit, &bad);
  return 0;
}
__attribute__((visibility("default"))) int nbls_sim_fr_quotient_roots(unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out_y32, uint8_t* out_q32,
                                                                      int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || (n && (!evals32 || !z32 || !out_y32 || !out_q32)) || (n << log2_n) > ((size_t)1 << 24)) return -1;
  const u32 N = 1u << log2_n, W = FR_EVAL_LANES;
  const std::vector<Fr> roots = sim_roots(log2_n);
  std::vector<Fr> part(W);
  std::vector<u32> pre((size_t)((N + W - 1) / W) * FR_NL * W);
  Fr y = fr_zero(); u32 hit = 0, bad = 0; int8_t st;
  for (size_t p = 0; p < n; p++)
    kzg_quotient_body(sim_wg<FR_EVAL_LANES>(), log2_n, evals32 + 32ull * N * p, z32 + 32ull * p, roots.data(), out_y32 + 32ull * p, out_q32 + 32ull * N * p, status ? status + p : &st,
                      pre.data(), part.data(), &y, &hit, &bad);
  return 0;
}
// nbls_fr_ntt (dir 0: to coefficients, 1: to values; a shift per polynomial or none)
__attribute__((visibility("default"))) int nbls_sim_fr_ntt(unsigned log2_n, int dir, size_t n, const uint8_t* in32, const uint8_t* shift32, uint8_t* out32, int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || (dir != 0 && dir != 1) || (n && (!in32 || !out32)) || (n << log2_n) > ((size_t)1 << 24)) return -1;
  sim_ntt(log2_n, dir == 0 ? FR_NTT_TO_COEFFS : FR_NTT_TO_EVALS, n, in32, shift32, 32, out32, nullptr, status);
  return 0;
}
// nbls_fr_ntt_large / nbls_fr_ntt_dev with the plan given (tail_bits / pass_bits 0: the engine's defaults): the bodies of kzg_ntt_pass_kernel and
// kzg_ntt_tail_kernel, launch after launch, one workgroup after another; out32 may equal in32
__attribute__((visibility("default"))) int nbls_sim_fr_ntt_large(unsigned log2_n, int dir, size_t n, const uint8_t* in32, const uint8_t* shift32, uint8_t* out32, int8_t* status,
                                                                 unsigned tail_bits, unsigned pass_bits) {
  const unsigned t = tail_bits ? tail_bits : FR_NTTL_DEFAULT_TAIL, P = pass_bits ? pass_bits : FR_NTTL_DEFAULT_PASS;
  if (log2_n < 1 || log2_n > FR_NTTL_MAX_LOG2 || (dir != 0 && dir != 1) || (n && (!in32 || !out32)) || (n << log2_n) > ((size_t)1 << 24) || n > ((size_t)1 << 24) ||
      t > FR_NTTL_MAX_TAIL || P > FR_NTTL_MAX_PASS || (log2_n > t && log2_n - t > 12))
    return -1;
  if (!n) return 0;
  const bool inverse = dir == 0;
  if (log2_n <= t) { sim_ntt(log2_n, inverse ? FR_NTT_TO_COEFFS : FR_NTT_TO_EVALS, n, in32, shift32, 32, out32, nullptr, status); return 0; }
  const unsigned K = log2_n - t, runs = fr_nttl_runs(K, P);
  const std::vector<Fr> roots = sim_roots(t), iroots = sim_inv_roots(t, roots), groots = sim_roots(K), table = inverse ? sim_inv_roots(K, groots) : groots;
  const Fr omega = fr_omega(log2_n), w = inverse ? fr_inv(omega) : omega;
  const size_t row = (size_t)32 << log2_n;
  std::vector<u32> flags(n, 0), a((size_t)8 << FR_NTTL_MAX_TILE);
  std::vector<Fr> sinv(n, fr_zero());
  Fr sh_s = fr_one();
  auto tails = [&](const uint8_t* src) {
    for (size_t blk = 0; blk < (n << K); blk++) {
      const size_t p = blk >> K, off = (blk * 32) << t;
      kzg_ntt_tail_body(sim_wg<FR_NTT_LANES>(), t, K, inverse, (u32)(blk & ((1u << K) - 1)), w, src + off, out32 + off, shift32 ? shift32 + 32 * p : nullptr, &sinv[p], roots.data(),
                        iroots.data(), &flags[p], status ? status + p : nullptr, a.data(), &sh_s);
    }
  };
  auto run = [&](unsigned i, const uint8_t* src) {
    const FrNttRun R = fr_nttl_run(log2_n, K, P, i);
    const unsigned lt = R.log2_n - R.j0 - R.q - R.c;
    const bool first = R.j0 == 0;
    for (size_t wgi = 0; wgi < (n << (lt + R.j0)); wgi++) {
      const u32 within = (u32)(wgi & ((1u << (lt + R.j0)) - 1));
      const size_t p = wgi >> (lt + R.j0);
      kzg_ntt_pass_body(sim_wg<FR_NTT_LANES>(), R, inverse, within >> lt, (within & ((1u << lt) - 1)) << R.c, within == 0, src + row * p, out32 + row * p,
                        first && !inverse && shift32 ? shift32 + 32 * p : nullptr, first && inverse && shift32 ? &sinv[p] : nullptr, table.data(), &flags[p],
                        first && inverse && status ? status + p : nullptr, a.data());
    }
  };
  if (inverse) { tails(in32); for (unsigned i = runs; i-- > 0;) run(i, out32); }
  else { for (unsigned i = 0; i < runs; i++) run(i, i ? out32 : in32); tails(out32); }
  return 0;
}
// nbls_kzg_compute_cells: the cells mode with the shift g for every blob; coef32 (may be NULL): the n x N coefficients the proofs read
__attribute__((visibility("default"))) int nbls_sim_kzg_cells(unsigned log2_n, size_t n, const uint8_t* blobs, uint8_t* out_cells, uint8_t* coef32, int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || (n && (!blobs || !out_cells)) || (n << log2_n) > ((size_t)1 << 24)) return -1;
  uint8_t g32[32];
  fr_to_bytes(fr_omega(log2_n + 1), g32);
  sim_ntt(log2_n, FR_NTT_CELLS, n, blobs, g32, 0, out_cells, coef32, status);
  return 0;
}
// kzg_canon_kernel: evals32 = n blobs, zeroed in place where an element is >= r; status: n bytes
__attribute__((visibility("default"))) int nbls_sim_kzg_canon(unsigned log2_n, size_t n, uint8_t* evals32, int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || (n && (!evals32 || !status))) return -1;
  u32 bad = 0;
  for (size_t p = 0; p < n; p++) kzg_canon_body(sim_wg<256>(), log2_n, evals32 + ((32 * p) << log2_n), status + p, &bad);
  return 0;
}
// kzg_sum_kernel: out32 = -(the sum of the n elements of v32, 32 bytes big-endian each) mod r
__attribute__((visibility("default"))) int nbls_sim_kzg_sum(size_t n, const uint8_t* v32, uint8_t* out32) {
  if ((n && !v32) || !out32 || n > ((size_t)1 << 24)) return -1;
  std::vector<Fr> v(n), part(FR_EVAL_LANES);
  for (size_t i = 0; i < n; i++) v[i] = fr_load_be(v32 + 32 * i);
  kzg_sum_body(sim_wg<FR_EVAL_LANES>(), (u32)n, v.data(), out32, part.data());
  return 0;
}
// the quotient rows of n blobs' cell proofs as kzg_cell_rows_kernel writes them: lane (blob, k, j) walks chain j of row k.  coef32: n x N coefficients; out_q32: n x
// (2 N / c) rows of N scalars.  -1 where the device call refuses the sizes (the table of the 2 N / c roots has at most 2^12 entries)
__attribute__((visibility("default"))) int nbls_sim_kzg_cell_rows(unsigned log2_n, unsigned log2_cell, size_t n, const uint8_t* coef32, uint8_t* out_q32) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12 || (n && (!coef32 || !out_q32))) return -1;
  const unsigned lm = log2_n + 1 - log2_cell;
  const std::vector<Fr> sroots = sim_roots(lm);
  for (uint64_t gid = 0; gid < ((uint64_t)n << (log2_n + 1)); gid++) {
    const u32 blob = (u32)(gid >> (log2_n + 1)), within = (u32)gid & ((2u << log2_n) - 1), k = within >> log2_cell, j = within & ((1u << log2_cell) - 1);
    const uint64_t row = ((uint64_t)blob << lm) + k;
    fr_cell_chain(coef32 + (((uint64_t)blob * 32) << log2_n), log2_n, log2_cell, j, sroots[k], out_q32 + ((row * 32) << log2_n));
  }
  return 0;
}
// The per-blob scalars of the FK20 cell proofs (kzg_fk20_scalars_kernel).  coef32: n x N coefficients; out32: n x M x c scalars, [blob][i][j]
__attribute__((visibility("default"))) int nbls_sim_kzg_fk20_scalars(unsigned log2_n, unsigned log2_cell, size_t n, const uint8_t* coef32, uint8_t* out32) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 11 || (n && (!coef32 || !out32)) || (n << log2_n) > ((size_t)1 << 24)) return -1;
  const unsigned lm = log2_n + 1 - log2_cell;
  const std::vector<Fr> sroots = sim_roots(lm);
  std::vector<u32> a(fr_fk_lds_words(lm));
  for (u32 b = 0; b < fr_fk_workgroups(lm, log2_cell, (u32)n); b++) kzg_fk20_scalars_body(sim_wg<FR_FK_LANES>(), log2_n, log2_cell, (u32)n, b, coef32, sroots.data(), out32, a.data());
  return 0;
}
// the projection matrix B of the FK20 cell proofs as kzg_fk20_matrix_kernel writes it: out32[(k M + i) * 32], M = 2^log2_m
__attribute__((visibility("default"))) int nbls_sim_kzg_fk20_matrix(unsigned log2_m, uint8_t* out32) {
  if (log2_m < 1 || log2_m > 11 || !out32) return -1;
  const std::vector<Fr> roots = sim_roots(log2_m), iroots = sim_inv_roots(log2_m, roots);
  for (u32 idx = 0; !(idx >> (2 * log2_m)); idx++) fr_store_q(fr_fk_matrix_entry(roots.data(), iroots.data(), log2_m, idx >> log2_m, idx & ((1u << log2_m) - 1)), out32 + 32ull * idx);
  return 0;
}
// The interpolation of n_cells cells as kzg_cell_interp_kernel runs it -- a re-enactment kept by hand: the kernel's lanes exchange registers, which the workgroup view does not
// model -- and kzg_cell_sum_kernel's body behind it in the sum mode: workgroups of FR_CELL_LANES lanes, lane groups of c lanes, every phase of a round on all lanes of a
// workgroup before the next, a stage's partner value read from the lane i ^ len of the same group, then fr_workgroup.h's tree.  n_wg: the workgroups of the launch (0: as many as the launcher takes).  sum == 0: out = the n_cells rows of
// c scalars -a_(k,i); else the c scalars -S_i.  pre, w32 (rows mode) and st_out may be NULL.  -1 where the device call refuses the sizes or an index
__attribute__((visibility("default"))) int nbls_sim_kzg_cell_interp(unsigned log2_n, unsigned log2_cell, size_t n_cells, int sum, unsigned n_wg, const uint8_t* cells,
                                                                    const uint32_t* cell_index, const int8_t* pre, const uint8_t* w32, uint8_t* out, int8_t* st_out) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > 6 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12 || !n_cells || n_cells > ((size_t)1 << 20) || !cells || !cell_index || !out ||
      (sum && !w32))
    return -1;
  const unsigned lm = log2_n + 1 - log2_cell;
  const u32 c = 1u << log2_cell, W = FR_CELL_LANES, n = (u32)n_cells;
  for (size_t k = 0; k < n_cells; k++) if (cell_index[k] >> lm) return -1;
  std::vector<Fr> iroots, ishifts((size_t)1 << lm);
  if (log2_cell) iroots = sim_inv_roots(log2_cell, sim_roots(log2_cell));
  const Fr g = fr_omega(log2_n + 1);
  for (u32 k = 0; k < (1u << lm); k++) ishifts[k] = fr_cell_ishift_entry(g, log2_n, lm, k);
  const u32 wgs = n_wg ? n_wg : fr_cell_workgroups(n, log2_cell, sum != 0), groups = (wgs * W) >> log2_cell, rounds = (n + groups - 1) / groups;
  std::vector<Fr> partial((size_t)wgs * c), v(W), nv(W), acc(W), part(W);
  std::vector<u32> bad(W);
  for (u32 b = 0; b < wgs; b++) {
    for (u32 t = 0; t < W; t++) acc[t] = fr_zero();
    for (u32 w = 0; w < rounds; w++) {
      auto cell_of = [&](u32 t, bool* valid) { const uint64_t k = (uint64_t)((b * W + t) >> log2_cell) + (uint64_t)w * groups; *valid = k < n; return *valid ? (u32)k : n - 1; };
      bool valid;
      for (u32 t = 0; t < W; t++) { v[t] = fr_load_q(cells + (((uint64_t)cell_of(t, &valid) << log2_cell) + (t & (c - 1))) * 32); bad[t] = fr_ge_r_mask(v[t]); }
      for (u32 m = 1; m < c; m <<= 1) { std::vector<u32> o(bad); for (u32 t = 0; t < W; t++) bad[t] = o[t] | o[t ^ m]; }
      for (u32 t = 0; t < W; t++) v[t] = fr_select(bad[t], fr_zero(), v[t]);
      for (u32 ll = 0; ll < log2_cell; ll++) {
        for (u32 t = 0; t < W; t++) nv[t] = fr_cell_stage(v[t], v[t ^ (1u << ll)], t & (c - 1), ll, log2_cell, iroots.data());
        v.swap(nv);
      }
      for (u32 t = 0; t < W; t++) {
        const u32 i = t & (c - 1), kk = cell_of(t, &valid);
        const int p = pre ? pre[kk] : 0;
        const u32 outm = bad[t] | ((u32)0 - (u32)(p != 0)) | ((u32)0 - (u32)!valid);
        const Fr a = fr_cell_coeff(v[t], ishifts[cell_index[kk]], i, log2_cell, outm);
        if (sum) acc[t] = fr_add(acc[t], fr_mul(a, fr_mul(fr_load_q(w32 + 32ull * kk), fr_r2())));
        else if (valid) fr_store_q(fr_neg(a), out + (((uint64_t)kk << log2_cell) + i) * 32);
        if (st_out && valid && i == 0) st_out[kk] = (int8_t)fr_cell_status(p, bad[t]);
      }
    }
    if (!sum) continue;
    part = acc;
    fr_tree(sim_wg<FR_CELL_LANES>(), part.data(), c);
    for (u32 t = 0; t < c; t++) partial[(size_t)b * c + t] = part[t];
  }
  if (sum) kzg_cell_sum_body(sim_wg<FR_CELL_LANES>(), log2_cell, wgs, partial.data(), out, part.data());
  return 0;
}
// nbls_kzg_recover_cells: the host's slot maps (fr_recover_slots), one lane per Z value (kzg_recover_z_kernel), then kzg_recover_kernel's body per blob, the half's coefficients
// S parked in the blob's coefficient row as on the device.  coef32 (may be NULL): the n x N coefficients the proofs read
__attribute__((visibility("default"))) int nbls_sim_kzg_recover(unsigned log2_n, unsigned log2_cell, size_t n, const uint32_t* cell_offsets, const uint32_t* cell_index,
                                                                const uint8_t* cells, uint8_t* out_cells, uint8_t* coef32, int8_t* status) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12) return -1;
  if (!n) return 0;
  if (!cell_offsets || !out_cells || cell_offsets[0] != 0 || (n << log2_n) > ((size_t)1 << 24)) return -1;
  for (size_t i = 0; i < n; i++) if (cell_offsets[i + 1] < cell_offsets[i]) return -1;
  if (cell_offsets[n] && (!cell_index || !cells)) return -1;
  const unsigned lm = log2_n + 1 - log2_cell;
  const u32 M = 1u << lm, per = M + M / 2;
  const std::vector<Fr> roots = sim_roots(log2_n), iroots = sim_inv_roots(log2_n, roots), sroots = sim_roots(lm);
  const FrRecoverConsts kc = fr_recover_consts(log2_n, log2_cell);
  std::vector<Fr> zv(per);
  std::vector<u32> slot(M), a((size_t)FR_NL << log2_n);
  std::vector<uint8_t> own((size_t)32 << log2_n);
  u32 bad = 0, diff = 0; int8_t st;
  for (size_t p = 0; p < n; p++) {
    const u32 first = cell_offsets[p];
    const int pre = fr_recover_slots(cell_index ? cell_index + first : nullptr, first, cell_offsets[p + 1] - first, lm, slot.data());
    if (!pre) for (u32 v = 0; v < per; v++) zv[v] = fr_recover_z(sroots.data(), slot.data(), lm, v, kc.c7);
    kzg_recover_body(sim_wg<FR_NTT_LANES>(), log2_n, log2_cell, cells, slot.data(), pre, zv.data(), kc, roots.data(), iroots.data(), out_cells + ((64 * p) << log2_n),
                     coef32 ? coef32 + ((32 * p) << log2_n) : own.data(), status ? status + p : &st, a.data(), &bad, &diff);
  }
  return 0;
}
// nbls_groth16_input_sums as g16_input_sums_kernel runs it -- a re-enactment kept by hand: the wavefront's OR is a cross-lane operation, which the workgroup view does not
// model: per tile of columns and workgroup of rows the G16_GROUPS wavefronts row after row -- every lane's look at the row, the wavefront's OR of the lanes' canonical checks,
// the masked product into the lane's accumulator --, ONE reduction per lane, fr_workgroup.h's tree, the partial rows; then g16_sum_kernel's body per tile.  n_wg: the workgroups per tile (0: as many as the launcher takes).  pre and status may be NULL.
// Returns -1 under the rules of the device call that need no context (a weight >= 2^64 among them)
__attribute__((visibility("default"))) int nbls_sim_g16_input_sums(size_t n, size_t m, unsigned n_wg, const uint8_t* inputs32, const uint8_t* weights32, const int8_t* pre,
                                                                   uint8_t* out32, int8_t* status) {
  if (!n || !m || !inputs32 || !weights32 || !out32 || n > G16_MAX_ELEMS || m > G16_MAX_ELEMS || n * m > G16_MAX_ELEMS) return -1;
  for (size_t i = 0; i < n; i++) for (int k = 0; k < 24; k++) if (weights32[32 * i + k]) return -1;
  const u32 M = (u32)m, tiles = g16_tiles(M), wgs = n_wg ? n_wg : g16_workgroups((u32)n), groups = wgs * G16_GROUPS, W = G16_LANES, T = G16_TILE;
  std::vector<Fr> partial((size_t)wgs * (m + 1)), part(W), x(T);
  std::vector<G16Acc> acc(W);
  for (u32 tile = 0; tile < tiles; tile++) for (u32 b = 0; b < wgs; b++) {
    for (u32 t = 0; t < W; t++) acc[t] = g16_acc_zero();
    for (u32 g = 0; g < G16_GROUPS; g++) for (uint64_t i = b * G16_GROUPS + g; i < n; i += groups) {
      u32 bad = 0;
      for (u32 lane = 0; lane < T; lane++) { u32 bl; x[lane] = g16_row_lane(inputs32 + i * m * 32, M, tiles, tile, lane, &bl); bad |= bl; }
      const int p = pre ? pre[i] : 0;
      for (u32 lane = 0; lane < T; lane++) g16_row_add(acc[g * T + lane], x[lane], weights32 + 32 * i, bad | ((u32)0 - (u32)(p != 0)));
      if (status && tile == 0) status[i] = (int8_t)g16_row_status(p, bad);
    }
    for (u32 t = 0; t < W; t++) part[t] = g16_reduce(acc[t]);
    fr_tree(sim_wg<G16_LANES>(), part.data(), T);
    for (u32 t = 0; t < T; t++) if (tile * T + t <= M) partial[(size_t)b * (m + 1) + tile * T + t] = part[t];
  }
  for (u32 tile = 0; tile < tiles; tile++) g16_sum_body(sim_wg<G16_LANES>(), M, tile, wgs, partial.data(), out32, part.data());
  return 0;
}
// ---- The Groth16 prover's kernels (groth16_prove_kernels.hip; the lane code is g16p_exec.h's, the text the device compiles).
// g16p_witness_kernel and g16p_spmv_kernel on one witness.  mats: rows, cols, vals32 of A, of B, of C as nbls_groth16_pk_create takes them (n_constraints + 1 offsets,
// canonical coefficients); w32: z | r | s; row_wave: the threshold (0: the default).  The launch is re-enacted wavefront by wavefront: the rows ordered by length as the key
// orders them, the first n_wave a wavefront each -- 64 shares, then the six levels of the cross-lane sum as the shuffles pair the lanes --, the others a lane each, in the
// simulator's lane order.  -> v32: a | b | c, values at rev(j); flags2: non-canonical, unsatisfied.  -1 under pk_create's rules on the matrices
__attribute__((visibility("default"))) int nbls_sim_g16p_spmv(unsigned log2_n, size_t n_vars, size_t n_constraints, const void* const mats[9], const uint8_t* w32, unsigned row_wave,
                                                              uint8_t* v32, uint8_t* flags2) {
  if (log2_n < 1 || log2_n > 21 || !n_vars || !mats || !w32 || !v32 || !flags2 || n_constraints > ((size_t)1 << log2_n)) return -1;
  const u32 N = 1u << log2_n, W = G16P_WAVE;
  std::vector<u32> rows[3]; std::vector<Fr> vals[3]; G16pMatrix M[3];
  for (int k = 0; k < 3; k++) {
    const u32 *r = (const u32*)mats[3 * k], *c = (const u32*)mats[3 * k + 1]; const uint8_t* v = (const uint8_t*)mats[3 * k + 2];
    if (!r || r[0] != 0) return -1;
    for (size_t j = 0; j < n_constraints; j++) if (r[j + 1] < r[j]) return -1;
    const u32 nnz = r[n_constraints];
    if (nnz && (!c || !v)) return -1;
    rows[k].assign((size_t)N + 1, nnz);
    for (size_t j = 0; j <= n_constraints; j++) rows[k][j] = r[j];
    vals[k].resize(nnz);
    for (u32 e = 0; e < nnz; e++) {
      if (c[e] >= n_vars || fr_ge_r_mask(fr_load_be(v + 32ull * e))) return -1;
      vals[k][e] = fr_from_bytes(v + 32ull * e);
    }
    M[k] = G16pMatrix{rows[k].data(), c, vals[k].data()};
  }
  std::vector<u32> len(N), order(N);
  for (u32 j = 0; j < N; j++) {
    len[j] = 0;
    for (int k = 0; k < 3; k++) if (rows[k][j + 1] - rows[k][j] > len[j]) len[j] = rows[k][j + 1] - rows[k][j];
    order[j] = j;
  }
  std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return len[x] > len[y]; });
  const u32 T = row_wave ? row_wave : (u32)G16P_ROW_WAVE_DEFAULT;
  u32 n_wave = 0;
  while (n_wave < N && len[order[n_wave]] >= T) n_wave++;
  uint8_t flags[G16P_FLAGS] = {0};
  std::vector<Fr> z(n_vars);
  for (uint64_t i = 0; i < n_vars + 2; i++) { const uint64_t e = g_lanes_down ? n_vars + 1 - i : i; g16p_witness_element(n_vars, e, w32, z.data(), flags); }
  const uint64_t waves = (uint64_t)n_wave + ((uint64_t)N - n_wave + W - 1) / W;
  for (uint64_t wave = 0; wave < waves; wave++) {
    if (wave < n_wave) {
      const u32 row = order[wave];
      Fr p[3][G16P_WAVE], q[G16P_WAVE];
      for (int k = 0; k < 3; k++) {
        for (u32 l = 0; l < W; l++) { const u32 lane = g_lanes_down ? W - 1 - l : l; p[k][lane] = g16p_row_part(M[k], z.data(), row, lane, W); }
        for (u32 m = 1; m < W; m <<= 1) { for (u32 l = 0; l < W; l++) q[l] = fr_add(p[k][l], p[k][l ^ m]); for (u32 l = 0; l < W; l++) p[k][l] = q[l]; }
      }
      g16p_row_store(log2_n, row, p[0][0], p[1][0], p[2][0], v32, flags);
      continue;
    }
    for (u32 l = 0; l < W; l++) {
      const u32 lane = g_lanes_down ? W - 1 - l : l;
      const uint64_t k = (wave - n_wave) * W + lane + n_wave;
      if (k >= N) continue;
      const u32 row = order[k];
      g16p_row_store(log2_n, row, g16p_row_part(M[0], z.data(), row, 0, 1), g16p_row_part(M[1], z.data(), row, 0, 1), g16p_row_part(M[2], z.data(), row, 0, 1), v32, flags);
    }
  }
  flags2[0] = flags[G16P_F_NONCANON]; flags2[1] = flags[G16P_F_UNSAT];
  return 0;
}
// nbls_groth16_quotient: g16p_check_kernel, the transforms of nbls_sim_fr_ntt_large with the plan given (tail_bits / pass_bits as there), g16p_quotient_kernel between
// them, the closing statuses.  status may be NULL
__attribute__((visibility("default"))) int nbls_sim_g16p_quotient(unsigned log2_n, size_t n, const uint8_t* a32, const uint8_t* b32, const uint8_t* c32, uint8_t* out_h32, int8_t* status,
                                                                  unsigned tail_bits, unsigned pass_bits) {
  const unsigned t = tail_bits ? tail_bits : FR_NTTL_DEFAULT_TAIL;
  if (log2_n < 1 || log2_n > 22 || (log2_n > t && log2_n - t > 12) || (n << log2_n) > ((size_t)1 << 24) || n > ((size_t)1 << 24) || (n && (!a32 || !b32 || !c32 || !out_h32))) return -1;
  if (!n) return 0;
  const size_t elems = n << log2_n, qb = elems * 32;
  std::vector<uint8_t> v[3] = {std::vector<uint8_t>(a32, a32 + qb), std::vector<uint8_t>(b32, b32 + qb), std::vector<uint8_t>(c32, c32 + qb)}, shift(n * 32, 0), violated(n, 0);
  std::vector<int8_t> st3(3 * n, 0);
  for (size_t i = 0; i < n; i++) shift[32 * i + 31] = 7;
  for (size_t i = 0; i < elems; i++) g16p_check_element(log2_n, g_lanes_down ? elems - 1 - i : i, a32, b32, c32, violated.data());
  for (int k = 0; k < 3; k++) if (nbls_sim_fr_ntt_large(log2_n, 0, n, v[k].data(), nullptr, v[k].data(), st3.data() + k * n, tail_bits, pass_bits)) return -1;
  for (int k = 0; k < 3; k++) if (nbls_sim_fr_ntt_large(log2_n, 1, n, v[k].data(), shift.data(), v[k].data(), nullptr, tail_bits, pass_bits)) return -1;
  const Fr kinv = g16p_quot_factor(log2_n);
  for (size_t i = 0; i < elems; i++) g16p_quot_element(log2_n, n, g_lanes_down ? elems - 1 - i : i, v[0].data(), v[1].data(), v[2].data(), st3.data(), kinv);
  if (nbls_sim_fr_ntt_large(log2_n, 0, n, v[0].data(), shift.data(), out_h32, nullptr, tail_bits, pass_bits)) return -1;
  if (status) for (size_t i = 0; i < n; i++) status[i] = (int8_t)g16p_quot_status(n, i, st3.data(), violated.data());
  return 0;
}
// g16p_scalars_kernel on one witness: w32 = z | r | s, h32 = the N coefficients of the quotient, one mask byte per query point, flags2 = non-canonical, unsatisfied
// -> sa, sb (n_vars + 2 scalars each), sc (n_aux + N + 2)
__attribute__((visibility("default"))) int nbls_sim_g16p_scalars(unsigned log2_n, size_t n_vars, size_t n_public, const uint8_t* w32, const uint8_t* h32, const uint8_t* mask_a,
                                                                 const uint8_t* mask_b, const uint8_t* mask_l, const uint8_t* flags2, uint8_t* sa, uint8_t* sb, uint8_t* sc) {
  if (log2_n < 1 || log2_n > 21 || !n_public || n_vars <= n_public || !w32 || !h32 || !mask_a || !mask_b || (n_vars - n_public - 1 && !mask_l) || !flags2 || !sa || !sb || !sc) return -1;
  uint8_t flags[G16P_FLAGS] = {0};
  flags[G16P_F_NONCANON] = flags2[0]; flags[G16P_F_UNSAT] = flags2[1];
  const G16pScalars S{n_vars, n_public, (uint64_t)1 << log2_n, w32, h32, mask_a, mask_b, mask_l, flags, sa, sb, sc};
  const uint64_t count = g16p_scalar_count(n_vars, n_public, S.N);
  for (uint64_t i = 0; i < count; i++) g16p_scalar_element(S, g_lanes_down ? count - 1 - i : i);
  return 0;
}
__attribute__((visibility("default"))) int nbls_sim_program_count() { return (int)P_COUNT; }
__attribute__((visibility("default"))) void nbls_sim_stats() { for (int i = 0; i < P_COUNT; i++) print_stats(get_program((ProgId)i)); }
}
