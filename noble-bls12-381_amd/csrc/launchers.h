// launchers.h -- the host entry of every kernel file: one declaration per launcher, included by the runtime that calls it (nbls_internal.h) AND by the .hip file that defines
// it, so that a definition which drifts from its declaration in an argument's type, order or count stops the build ("conflicting types") instead of linking -- with C linkage
// the symbol carries no types.  Word arrays, the stream and the status arrays that both sides hold as such have their real types; byte arrays and arrays of 16-byte vectors
// are void*, cast once, inside the launcher (so are the message offsets of nbls_xmd_launch, which every caller carves from a byte block or receives as void*).  Every
// launcher returns 0 or a hipError_t, enqueues nothing for zero items, and has hidden visibility (csrc/Makefile).
// (nbls_aot_launch: aot.h, next to the argument block it takes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbls { struct KernelArgs; struct FrNttRun; struct G16pScalars; }

extern "C" {
// vm_kernel.hip, vm_wide_kernel.hip
int nbls_vm_launch(const nbls::KernelArgs* ka, unsigned lds_bytes, hipStream_t stream);
int nbls_vm_wide_launch(const nbls::KernelArgs* ka, unsigned lds_bytes, hipStream_t stream);
int nbls_fp_inv_wide_launch(unsigned n, const void* in, void* out, hipStream_t stream);   // fp_inv_wide.h: four elements per wavefront, one limb per lane
// g1_wide.h: `sums` times sum_w 2^(shift w) S_w over nwin points, one wavefront each
int nbls_g1_wide_combine_launch(const void* S, int nwin, int shift, void* out, unsigned sums, hipStream_t stream);
// pow_kernels.hip
int nbls_fp_inv_launch(unsigned n, const void* in, void* out, unsigned prio, hipStream_t stream);   // prio: issue priority of the launch's wavefronts, 0 .. 3
int nbls_fp_pow_launch(unsigned n, const void* in, void* out, const uint8_t* ops, int nops, void* scratch, int is_fp2, hipStream_t stream);
int nbls_pow_wide_launch(unsigned n, const void* in, void* out, const uint8_t* ops, int nops, int is_fp2, hipStream_t stream);
int nbls_flag_compact_launch(unsigned n, const void* flags, uint32_t* list, uint32_t* count, hipStream_t stream);
// xmd_kernel.hip
int nbls_xmd_launch(unsigned n, const void* msgs, const void* offsets, const void* dst, unsigned dst_len, void* out, unsigned len_in_bytes, uint32_t* bad_flag, hipStream_t stream);
// rlc_kernels.hip
int nbls_rlc_weights_launch(unsigned n, const void* seed32, void* out, hipStream_t stream);
int nbls_rlc_interleave_launch(unsigned n, const uint32_t* msg_index, const void* pk96, const void* neg_g1, const void* h192, const void* sig192, void* g1x, void* g2x,
                               hipStream_t stream);
int nbls_rlc_is_one_launch(unsigned n, const void* f576, void* ok, hipStream_t stream);
// agg_kernels.hip
int nbls_agg_keys_launch(unsigned nkeys, unsigned n, const uint32_t* koff, const uint32_t* index, const int8_t* st_src, uint32_t* set_id, uint32_t* rank, int8_t* st,
                         uint32_t* first_bad, hipStream_t stream);
int nbls_agg_points_launch(size_t nkeys, unsigned elem_bytes, const uint32_t* index, const void* st, const void* ident, const void* src, void* dst, hipStream_t stream);
int nbls_agg_status_launch(unsigned n, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out, hipStream_t stream);
int nbls_agg_fix_zero_launch(unsigned n, const void* zero, const void* fixed96, void* pts96, uint32_t* flag, hipStream_t stream);
// fr_kernels.hip
int nbls_fr_op_launch(unsigned n, int op, const void* a32, const void* b32, void* out32, void* status, hipStream_t stream);
int nbls_fr_lagrange_launch(unsigned n, unsigned ngroups, const uint32_t* off, const void* ids32, void* X, void* L, uint32_t* group_of, uint32_t* bad_group, void* out32,
                            hipStream_t stream);
int nbls_fr_combine_status_launch(unsigned ngroups, unsigned out_bytes, const uint32_t* bad_group, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out,
                                  void* status, hipStream_t stream);
int nbls_fr_group_status_launch(unsigned ngroups, const uint32_t* bad_group, void* status, hipStream_t stream);
// poly_kernels.hip
int nbls_poly_group_launch(unsigned n, unsigned ngroups, const uint32_t* off, uint32_t* group_of, hipStream_t stream);
int nbls_poly_coef_launch(size_t items, unsigned elem_bytes, unsigned j, const uint32_t* group_of, const uint32_t* coff, const void* ident, const void* pts, void* dst,
                          hipStream_t stream);
int nbls_poly_status_launch(unsigned n, unsigned out_bytes, const uint32_t* group_of, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out, void* status,
                            hipStream_t stream);
// msm_kernels.hip
int nbls_msm_keys_launch(unsigned m, unsigned dims, unsigned nwin, unsigned c, unsigned i0, unsigned g0, unsigned ngroups, unsigned n_pts, const uint32_t* off,
                         const void* scalars, uint32_t* keys, uint32_t* vals, hipStream_t stream);
int nbls_msm_keys_map_launch(unsigned m, unsigned dims, unsigned nwin, unsigned c, unsigned i0, unsigned g0, unsigned ngroups, unsigned n_pts, unsigned glen, unsigned pt_block,
                             unsigned k_mod, const void* scalars, uint32_t* keys, uint32_t* vals, hipStream_t stream);
int nbls_msm_decompose_launch(unsigned n, unsigned dims, const void* scalars, void* out, hipStream_t stream);
int nbls_msm_sac_launch(unsigned n, const void* scalars, void* out, hipStream_t stream);
int nbls_msm_sort_launch(void* temp, size_t* temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t m, int key_bits,
                         hipStream_t stream);
int nbls_msm_gather_launch(size_t m, unsigned elem_bytes, const uint32_t* idx, const void* src, void* dst, hipStream_t stream);
int nbls_msm_rank_launch(void* temp, size_t* temp_bytes, size_t m, const uint32_t* keys, uint32_t* pos, uint32_t* maxrun, hipStream_t stream);
int nbls_msm_pairs_launch(size_t m, unsigned d, const uint32_t* keys, const uint32_t* pos, uint32_t* list, uint32_t* count, hipStream_t stream);
int nbls_msm_fill_launch(size_t count, unsigned elem_bytes, const void* ident, void* dst, hipStream_t stream);
int nbls_msm_heads_launch(size_t m, unsigned elem_bytes, const uint32_t* keys, const void* P, void* buckets, hipStream_t stream);
int nbls_msm_bitsel_launch(size_t nbw, unsigned c, unsigned elem_bytes, const void* buckets, void* G, hipStream_t stream);
// kzg_kernels.hip
int nbls_kzg_roots_launch(unsigned log2_n, void* table, hipStream_t stream);
int nbls_kzg_eval_launch(unsigned log2_n, unsigned n, const void* evals32, const void* z32, const void* roots, void* out32, void* status, hipStream_t stream);
int nbls_kzg_items_launch(unsigned n, const void* dst, const void* w32, const void* z32, const void* y32, const void* yst, const void* gen96, void* aff, void* s1, void* s2,
                          void* t, void* pre, hipStream_t stream);
int nbls_kzg_item_scalars_launch(unsigned n, const void* pre, const void* dst, const void* z32, const void* y32, void* zs, void* ny, hipStream_t stream);
int nbls_kzg_item_status_launch(unsigned n, const void* pre, const void* pst, const void* xzero, const void* one, void* status, hipStream_t stream);
int nbls_kzg_quotient_launch(unsigned log2_n, unsigned n, const void* evals32, const void* z32, const void* roots, void* out_y32, void* out_q32, void* status,
                             hipStream_t stream);
int nbls_kzg_canon_launch(unsigned log2_n, unsigned n, void* evals32, void* status, hipStream_t stream);
int nbls_kzg_prove_tail_launch(unsigned n, const void* zero, const void* st_a, const void* st_b, void* out48, void* status, hipStream_t stream);
int nbls_kzg_inv_roots_launch(unsigned log2_n, const void* roots, void* table, hipStream_t stream);
int nbls_kzg_ntt_launch(unsigned log2_n, unsigned mode, unsigned n, const void* in32, const void* shift32, unsigned shift_stride, const void* roots, const void* iroots,
                        void* out32, void* coef32, void* status, hipStream_t stream);
int nbls_kzg_ntt_pass_launch(const nbls::FrNttRun* run, unsigned inverse, unsigned n, const void* in32, void* out32, const void* shift32, const void* sinv, const void* table,
                             void* flags, void* status, hipStream_t stream);
int nbls_kzg_ntt_tail_launch(unsigned log2_t, unsigned log2_k, unsigned inverse, unsigned n, const uint32_t* w32, const void* in32, void* out32, const void* shift32, void* sinv,
                             const void* roots, const void* iroots, void* flags, void* status, hipStream_t stream);
int nbls_kzg_cell_rows_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* coef32, const void* sroots, const void* blob_st, void* out_q32, void* row_st,
                              hipStream_t stream);
int nbls_kzg_fk20_scalars_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* coef32, const void* sroots, void* out32, hipStream_t stream);
int nbls_kzg_fk20_row_status_launch(unsigned log2_m, unsigned n, const void* blob_st, void* row_st, hipStream_t stream);
int nbls_kzg_fk20_powers_launch(unsigned log2_n, unsigned log2_cell, const void* sroots, void* out32, hipStream_t stream);
int nbls_kzg_fk20_matrix_launch(unsigned log2_m, const void* sroots, const void* isroots, void* out32, hipStream_t stream);
int nbls_kzg_cell_ishifts_launch(unsigned log2_n, unsigned log2_m, void* table, hipStream_t stream);
int nbls_kzg_recover_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* cells, const uint32_t* slot, const void* pre, const void* sroots, const void* consts,
                            const void* roots, const void* iroots, void* zv, void* out32, void* coef32, void* status, hipStream_t stream);
int nbls_kzg_cell_interp_launch(unsigned log2_cell, unsigned n_cells, int sum, const void* cells, const uint32_t* cell_index, const void* pre, const void* w32, const void* iroots,
                                const void* ishifts, void* rows32, void* partial, void* out32, void* st_out, hipStream_t stream);
int nbls_kzg_cell_pre_launch(unsigned n, const void* dstc, const void* dstp, const uint32_t* ci, void* pre0, hipStream_t stream);
int nbls_kzg_cell_items_launch(unsigned n, const void* dstc, const void* dstp, const uint32_t* ci, const uint32_t* cell_index, const void* pre, const void* w32, const void* sroots,
                               const void* gen96, const void* affc, void* affp, void* gath, void* gst, void* s1, void* s2, void* s3, void* zs, hipStream_t stream);
// groth16_kernels.hip
int nbls_g16_input_sums_launch(unsigned n, unsigned m, const void* inputs32, const void* w32, const void* pre, void* partial, void* out32, void* st_out, hipStream_t stream);
int nbls_g16_split_launch(unsigned n, const void* proofs192, void* ac48, void* b96, hipStream_t stream);
int nbls_g16_pre_launch(unsigned n, const void* sta, const void* stb, const void* stc, void* pre0, hipStream_t stream);
int nbls_g16_items_launch(unsigned n, const void* pre, const void* w32, const void* gen96, const void* g2_192, void* a96, void* c96, void* b192, void* s1, hipStream_t stream);
int nbls_g16_rows_launch(unsigned n, unsigned m, const void* pre, void* rows32, hipStream_t stream);
int nbls_g16_status_launch(unsigned n, const void* pre, const void* one, void* status, hipStream_t stream);
int nbls_g16_prepare_tail_launch(unsigned n, const void* zero, const void* pre, void* out48, void* status, hipStream_t stream);
// groth16_prove_kernels.hip
int nbls_g16p_witness_launch(size_t n_vars, const void* w32, void* z, void* flags, hipStream_t stream);
int nbls_g16p_spmv_launch(unsigned log2_n, unsigned n_wave, const uint32_t* order, const void* const mats[9], const void* z, void* v32, void* flags, hipStream_t stream);
int nbls_g16p_quotient_launch(unsigned log2_n, size_t n, void* a32, const void* b32, const void* c32, const void* st3, const uint32_t* kinv, hipStream_t stream);
int nbls_g16p_check_launch(unsigned log2_n, size_t n, const void* a32, const void* b32, const void* c32, void* violated, hipStream_t stream);
int nbls_g16p_quot_status_launch(size_t n, const void* st3, const void* violated, void* status, hipStream_t stream);
int nbls_g16p_scalars_launch(const nbls::G16pScalars* S, hipStream_t stream);
int nbls_g16p_mask_launch(size_t n, unsigned elem_bytes, const void* st, const void* fixed, void* pts, void* mask, hipStream_t stream);
int nbls_g16p_finish_launch(const void* flags, const void* zero3, void* out192, void* status, hipStream_t stream);
}
