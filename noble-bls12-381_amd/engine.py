"""ctypes binding of libnbls.so (include/nbls.h).  Mirrors the reference's batched entry points:
pairing (index.ts:715), the Miller-product core of verify/verifyBatch (index.ts:763-766, 811-816) and
Fp12.finalExponentiate (math.ts:856).

A process that also uses PyTorch-ROCm must import torch BEFORE the first Engine is created: the torch wheel bundles its own HIP
runtime, libnbls.so binds to whichever runtime is already loaded, and torch loaded second reports "No HIP GPUs are available"."""
import ctypes as C
import os
try:
    import numpy as _np
except ImportError:      # the binding itself needs only ctypes
    _np = None

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 5   # include/nbls.h NBLS_ABI_VERSION: checked at load (round 4's advisor: an ABI-1 caller of *_partial read stale bytes from an ABI-2 library with no error)
PROGRAMS = []   # names of the step programs in the library's numbering (filled by load_library from nbls_program_name)
DST_DEFAULT = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'   # htfDefaults.DST, reference index.ts:64


class NblsError(RuntimeError):
    pass


def lib_path():
    return os.environ.get('NBLS_LIBRARY') or os.path.join(_HERE, 'libnbls.so')   # NBLS_LIBRARY: explicit path of the engine library


class Groth16PkDesc(C.Structure):
    """nbls_groth16_pk_desc (include/nbls.h): the R1CS matrices in CSR form and the proving key's compressed points"""
    _fields_ = ([('log2_n', C.c_uint), ('n_vars', C.c_size_t), ('n_public', C.c_size_t), ('n_constraints', C.c_size_t)] +
                [(m + f, C.c_void_p) for m in 'abc' for f in ('_rows', '_cols', '_vals32')] +
                [(f, C.c_void_p) for f in ('alpha_g1_48', 'beta_g1_48', 'beta_g2_96', 'delta_g1_48', 'delta_g2_96', 'a_query48', 'b_g1_query48', 'b_g2_query96', 'l_query48', 'h_query48')])


def load_library():
    p = lib_path()
    if not os.path.exists(p):
        raise NblsError('libnbls.so is not built (run __graft_entry__.build() or make -C noble-bls12-381_amd/csrc)')
    lib = C.CDLL(p)
    lib.nbls_strerror.restype = C.c_char_p
    lib.nbls_config_describe.restype = C.c_char_p
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    lib.nbls_init.argtypes = [i32, C.POINTER(vp)]
    lib.nbls_destroy.argtypes = [vp]
    lib.nbls_last_hip_error.argtypes = [vp]
    lib.nbls_device_synchronize.argtypes = [vp]
    lib.nbls_pairing_batch.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp]
    lib.nbls_pairing_batch_dev.argtypes = [vp, sz, vp, vp, i32, vp, vp]
    lib.nbls_miller_product.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp]
    lib.nbls_miller_product_dev.argtypes = [vp, sz, vp, vp, i32, vp, vp]
    lib.nbls_final_exp_batch.argtypes = [vp, sz, vp, vp]
    lib.nbls_final_exp_batch_dev.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_fp12_product_final_dev.argtypes = [vp, sz, vp, i32, vp, vp]
    lib.nbls_program_stats.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    lib.nbls_g1_validate_batch.argtypes = [vp, sz, vp, vp]
    lib.nbls_g2_validate_batch.argtypes = [vp, sz, vp, vp]
    lib.nbls_g1_decompress_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_g2_decompress_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_hash_to_g2_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp]
    lib.nbls_hash_to_g1_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp]
    lib.nbls_encode_to_g1_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp]
    lib.nbls_encode_to_g2_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp]
    lib.nbls_g1_sum.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_g2_sum.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_g1_compress_batch.argtypes = [vp, sz, vp, vp]
    lib.nbls_g2_compress_batch.argtypes = [vp, sz, vp, vp]
    lib.nbls_g1_mul_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.nbls_g2_mul_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.nbls_g1_msm.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.nbls_g2_msm.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.nbls_msm_dev.argtypes = [vp, i32, sz, vp, vp, C.c_uint32, vp, vp, vp]
    lib.nbls_g1_msm_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_g2_msm_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_g1_msm_rows.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    lib.nbls_g2_msm_rows.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    lib.nbls_sign_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp]
    lib.nbls_sign_batch_dev.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.nbls_verify_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.POINTER(i32)]
    lib.nbls_verify_multiple.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_verify_aggregates.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_verify_aggregates_indexed.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_verify_multiple_shared.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_verify_aggregates_shared.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_verify_aggregates_indexed_shared.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(i32), vp]
    lib.nbls_fr_op_batch.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    lib.nbls_lagrange_at_zero.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.nbls_g2_combine_shares.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_g1_combine_shares.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_g1_poly_eval.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nbls_g2_poly_eval.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nbls_fr_eval_roots.argtypes = [vp, C.c_uint, sz, vp, vp, vp, vp]
    lib.nbls_kzg_verify_proofs.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp]
    lib.nbls_kzg_verify_blobs.argtypes = [vp, C.c_uint, sz, vp, vp, vp, vp, vp, C.POINTER(i32), vp]
    lib.nbls_kzg_setup_create.argtypes = [vp, C.c_uint, vp, vp, C.POINTER(vp)]
    lib.nbls_kzg_setup_destroy.argtypes = [vp]
    lib.nbls_kzg_setup_destroy.restype = None
    lib.nbls_kzg_setup_log2n.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.nbls_fr_quotient_roots.argtypes = [vp, C.c_uint, sz, vp, vp, vp, vp, vp]
    lib.nbls_kzg_commit_blobs.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.nbls_kzg_compute_proofs.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_kzg_compute_blob_proofs.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.nbls_fr_ntt.argtypes = [vp, C.c_uint, C.c_int, sz, vp, vp, vp, vp]
    lib.nbls_fr_ntt_large.argtypes = [vp, C.c_uint, C.c_int, sz, vp, vp, vp, vp]
    lib.nbls_fr_ntt_dev.argtypes = [vp, C.c_uint, C.c_int, sz, vp, vp, vp, vp, vp]
    lib.nbls_kzg_compute_cells.argtypes = [vp, C.c_uint, C.c_uint, sz, vp, vp, vp]
    lib.nbls_kzg_monomial_create.argtypes = [vp, C.c_uint, vp, vp, C.POINTER(vp)]
    lib.nbls_kzg_monomial_destroy.argtypes = [vp]
    lib.nbls_kzg_monomial_destroy.restype = None
    lib.nbls_kzg_monomial_log2n.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.nbls_kzg_compute_cells_and_proofs.argtypes = [vp, vp, C.c_uint, sz, vp, vp, vp, vp]
    lib.nbls_kzg_verify_cells.argtypes = [vp, vp, C.c_uint, sz, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp]
    lib.nbls_kzg_recover_cells.argtypes = [vp, C.c_uint, C.c_uint, sz, vp, vp, vp, vp, vp]
    lib.nbls_kzg_recover_cells_and_proofs.argtypes = [vp, vp, C.c_uint, sz, vp, vp, vp, vp, vp, vp]
    lib.nbls_kzg_fk20_create.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
    lib.nbls_kzg_fk20_destroy.argtypes = [vp]
    lib.nbls_kzg_fk20_destroy.restype = None
    lib.nbls_kzg_fk20_params.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    lib.nbls_kzg_compute_cells_and_proofs_fk20.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.nbls_kzg_recover_cells_and_proofs_fk20.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
    lib.nbls_groth16_vk_create.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    lib.nbls_groth16_vk_destroy.argtypes = [vp]
    lib.nbls_groth16_vk_destroy.restype = None
    lib.nbls_groth16_vk_inputs.argtypes = [vp, C.POINTER(sz)]
    lib.nbls_groth16_verify.argtypes = [vp, vp, sz, vp, vp, vp, C.POINTER(i32), vp]
    lib.nbls_groth16_prepare_inputs.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.nbls_groth16_input_sums.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp]
    lib.nbls_groth16_pk_create.argtypes = [vp, C.POINTER(Groth16PkDesc), vp, C.POINTER(vp)]
    lib.nbls_groth16_pk_destroy.argtypes = [vp]
    lib.nbls_groth16_pk_destroy.restype = None
    lib.nbls_groth16_pk_params.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(sz), C.POINTER(sz)]
    lib.nbls_groth16_pk_wiped.argtypes = [vp, vp, C.POINTER(i32)]
    lib.nbls_groth16_prove.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.nbls_groth16_quotient.argtypes = [vp, C.c_uint, sz, vp, vp, vp, vp, vp]
    lib.nbls_keyset_create.argtypes = [vp, sz, vp, vp, C.POINTER(vp)]
    lib.nbls_keyset_destroy.argtypes = [vp]
    lib.nbls_keyset_destroy.restype = None
    lib.nbls_keyset_size.argtypes = [vp, C.POINTER(sz)]
    lib.nbls_verify_batch_dev_inputs.argtypes = [vp, sz, vp, vp, vp, C.POINTER(i32), vp, vp]
    lib.nbls_verify_batch_msgs_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.POINTER(i32), vp]
    lib.nbls_verify_batch_partial_dev.argtypes = [vp, sz, vp, vp, vp, vp, C.POINTER(i32), vp, vp]
    lib.nbls_g2_prepare.argtypes = [vp, sz, vp, vp]
    lib.nbls_g2_prepare_dev.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_lines_to_wire_dev.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_lines_from_wire_dev.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_pairing_prepared_dev.argtypes = [vp, sz, vp, vp, sz, i32, vp, vp]
    lib.nbls_miller_product_prepared_dev.argtypes = [vp, sz, vp, vp, sz, i32, vp, vp]
    lib.nbls_pairing_prepared.argtypes = [vp, sz, vp, vp, sz, i32, i32, vp]
    lib.nbls_set_tuning.argtypes = [vp, i32, C.c_longlong]
    lib.nbls_field_kernel_raw.argtypes = [vp, i32, i32, sz, vp, vp]
    lib.nbls_map_uniform_batch.argtypes = [vp, i32, sz, vp, vp, vp]
    for nm in ('nbls_g1_from_hex_batch', 'nbls_g2_from_hex_batch', 'nbls_g2_from_signature_batch'):
        getattr(lib, nm).argtypes = [vp, sz, vp, sz, vp, vp]
    lib.nbls_g1_to_hex_batch.argtypes = [vp, sz, vp, vp, i32, vp]
    lib.nbls_g2_to_hex_batch.argtypes = [vp, sz, vp, vp, i32, vp]
    lib.nbls_g1_clear_cofactor_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_g2_clear_cofactor_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.nbls_init_multi.argtypes = [i32, C.POINTER(i32), C.POINTER(vp)]
    lib.nbls_destroy_multi.argtypes = [vp]
    lib.nbls_multi_device_count.argtypes = [vp]
    lib.nbls_multi_peer_access.argtypes = [vp, i32]
    lib.nbls_multi_pairing_batch.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp]
    lib.nbls_multi_miller_product.argtypes = [vp, sz, vp, vp, i32, i32, vp, vp]
    lib.nbls_multi_verify_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.POINTER(i32)]
    lib.nbls_program_name.restype = C.c_char_p
    lib.nbls_program_name.argtypes = [i32]
    lib.nbls_context_device.argtypes = [vp]
    lib.nbls_pool_init.argtypes = [i32, i32, C.POINTER(vp)]
    lib.nbls_pool_init_ex.argtypes = [i32, i32, C.c_uint, C.POINTER(vp)]
    lib.nbls_pool_stream_priority.argtypes = [vp, i32, C.POINTER(i32)]
    lib.nbls_pool_outstanding.argtypes = [vp, i32, C.POINTER(i32)]
    lib.nbls_pool_destroy.argtypes = [vp]
    lib.nbls_pool_depth.argtypes = [vp]
    lib.nbls_pool_context.restype = vp
    lib.nbls_pool_context.argtypes = [vp, i32]
    lib.nbls_pool_next_slot.argtypes = [vp]
    lib.nbls_pool_pairing_batch_dev.argtypes = [vp, sz, vp, vp, i32, vp, C.POINTER(i32)]
    lib.nbls_pool_synchronize.argtypes = [vp]
    lib.nbls_program_kernel.restype = C.c_char_p
    lib.nbls_program_kernel.argtypes = [vp, i32]
    lib.nbls_extra_program_kernel.restype = C.c_char_p
    lib.nbls_extra_program_kernel.argtypes = [vp, C.c_char_p]
    if lib.nbls_abi_version() != ABI_VERSION:
        raise NblsError('libnbls.so has ABI %d, this binding is written for ABI %d (rebuild: make -C noble-bls12-381_amd/csrc)' % (lib.nbls_abi_version(), ABI_VERSION))
    if not PROGRAMS:
        PROGRAMS.extend(lib.nbls_program_name(k).decode() for k in range(lib.nbls_program_count()))
    lib.nbls_timing_enable.argtypes = [vp, i32]
    lib.nbls_timing_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    return lib


def group_messages(msgs):
    """a flat list of messages -> (distinct, index): the distinct messages by byte equality in the order of their first appearance, and index[i] = the position of msgs[i] among
    them -- the (msgs, msg_index) arguments of Engine.verify_multiple_shared and its twins"""
    seen, distinct, index = {}, [], []
    for m in msgs:
        m = bytes(m)
        g = seen.get(m)
        if g is None:
            g = seen[m] = len(distinct)
            distinct.append(m)
        index.append(g)
    return distinct, index


class _DeviceHandle:
    """What the five handle classes below share: the library, the handle, close() / __del__ through the subclass's destroy function, and the read through one of its getters.
    _destroy: the name of the destroy function; _thing: what the closed-handle message calls the object"""
    _destroy = _thing = None

    def __init__(self, lib, handle):
        self.lib = lib
        self.h = handle

    def _get(self, getter, *ctypes_out):
        out = [t(0) for t in ctypes_out]
        if self.h is None or getattr(self.lib, getter)(self.h, *[C.byref(o) for o in out]) != 0:
            raise NblsError('%s: the %s is closed' % (type(self).__name__, self._thing))
        return [o.value for o in out]

    def close(self):
        if getattr(self, 'h', None):
            getattr(self.lib, self._destroy)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeySet(_DeviceHandle):
    """A table of decoded keys in device memory (nbls_keyset_create; Engine.create_keyset).  Freed by close() or when the object goes away."""
    _destroy, _thing = 'nbls_keyset_destroy', 'table'

    def __len__(self):
        return self._get('nbls_keyset_size', C.c_size_t)[0]


class KzgSetup(_DeviceHandle):
    """A trusted setup's Lagrange basis in device memory (nbls_kzg_setup_create; Engine.kzg_setup), decoded and split once.  Freed by close() or when the object goes away."""
    _destroy, _thing = 'nbls_kzg_setup_destroy', 'setup'

    @property
    def log2_n(self):
        return self._get('nbls_kzg_setup_log2n', C.c_uint)[0]


class KzgFk20Setup(_DeviceHandle):
    """The fixed part of the FK20 cell proofs for one (log2_n, log2_cell) in device memory (nbls_kzg_fk20_create; Engine.kzg_fk20_setup): the transformed stripes of the
    monomial basis and the projection matrix.  Usable from every Engine on its device.  Freed by close() or when the object goes away."""
    _destroy, _thing = 'nbls_kzg_fk20_destroy', 'setup'

    @property
    def log2_n(self):
        return self._get('nbls_kzg_fk20_params', C.c_uint, C.c_uint)[0]

    @property
    def log2_cell(self):
        return self._get('nbls_kzg_fk20_params', C.c_uint, C.c_uint)[1]


class KzgMonomialSetup(_DeviceHandle):
    """A trusted setup's monomial basis [tau^i]G1 in device memory (nbls_kzg_monomial_create; Engine.kzg_monomial_setup), decoded and split once.  Freed by close() or when the
    object goes away."""
    _destroy, _thing = 'nbls_kzg_monomial_destroy', 'setup'

    @property
    def log2_n(self):
        return self._get('nbls_kzg_monomial_log2n', C.c_uint)[0]


class Groth16Vk(_DeviceHandle):
    """A Groth16 verifying key in device memory (nbls_groth16_vk_create; Engine.groth16_vk): alpha, the line tables of -beta, -gamma, -delta and the IC points, decoded and
    converted once.  Usable from every Engine on its device.  Freed by close() or when the object goes away."""
    _destroy, _thing = 'nbls_groth16_vk_destroy', 'key'

    @property
    def inputs(self):
        return self._get('nbls_groth16_vk_inputs', C.c_size_t)[0]


class Groth16Pk(_DeviceHandle):
    """A Groth16 proving key in device memory (nbls_groth16_pk_create; Engine.groth16_pk): the R1CS matrices, the decoded query points as the arrays the sums read, and the
    workspace of a proof.  Usable from every Engine on its device, one proof at a time.  Freed by close() or when the object goes away."""
    _destroy, _thing = 'nbls_groth16_pk_destroy', 'key'

    def _params(self):
        return self._get('nbls_groth16_pk_params', C.c_uint, C.c_size_t, C.c_size_t)

    @property
    def log2_n(self):
        return self._params()[0]

    @property
    def n_vars(self):
        return self._params()[1]

    @property
    def n_public(self):
        return self._params()[2]


class KzgSetupError(NblsError):
    """nbls_kzg_setup_create refused the points: .code is the call's return code, .status the decoder's status of every entry (bytes)"""

    def __init__(self, msg, code, status):
        NblsError.__init__(self, msg)
        self.code, self.status = code, status


class Engine:
    """One engine context = one GPU."""

    def __init__(self, device_id=0, _handle=None):
        self.lib = load_library()
        self._owned = _handle is None
        if _handle is not None:      # a context owned by a pool / multi handle (nbls_pool_context, nbls_multi_context): not destroyed by this object
            self.h = C.c_void_p(_handle)
            self.device_id = self.lib.nbls_context_device(self.h)
            return
        h = C.c_void_p()
        r = self.lib.nbls_init(device_id, C.byref(h))
        if r != 0:
            raise NblsError('nbls_init failed: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r))
        self.h = h
        self.device_id = device_id

    def close(self):
        if getattr(self, 'h', None):
            if self._owned:
                self.lib.nbls_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != 0:
            raise NblsError('%s (code %d, hip %d)' % (self.lib.nbls_strerror(r).decode(), r, self.lib.nbls_last_hip_error(self.h)))

    # ---- host-buffer entry points (bytes in, bytes out)
    def pairing_batch(self, g1_aff, g2_aff, with_final_exp=True, validate=False):
        n = len(g1_aff) // 96
        assert len(g1_aff) == 96 * n and len(g2_aff) == 192 * n
        out = C.create_string_buffer(576 * n)
        st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_pairing_batch(self.h, n, g1_aff, g2_aff, int(with_final_exp), int(validate), out, st))
        return out.raw, st.raw[:n]

    def miller_product(self, g1_aff, g2_aff, final_exp=True, validate=False):
        n = len(g1_aff) // 96
        out = C.create_string_buffer(576)
        st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_miller_product(self.h, n, g1_aff, g2_aff, int(final_exp), int(validate), out, st))
        return out.raw, st.raw[:n]

    # ---- prepared G2 points (PointG2.pairingPrecomputes index.ts:703-711, PointG1.millerLoop index.ts:452-454)
    LINE_TABLE_BYTES = 26112
    LINE_WIRE_BYTES = 19584

    def g2_prepare(self, g2_aff):
        """n affine G2 points -> n line tables in wire form (68 x [Fp2, Fp2, Fp2] as Fp2.toBytes, 19,584 B each)"""
        n = len(g2_aff) // 192
        out = C.create_string_buffer(max(self.LINE_WIRE_BYTES * n, 1))
        self._chk(self.lib.nbls_g2_prepare(self.h, n, g2_aff, out))
        return out.raw[:self.LINE_WIRE_BYTES * n]

    def pairing_prepared(self, g1_aff, tables_wire, with_final_exp=True, product=False):
        """n G1 points against n (or 1) prepared tables: n pairings, or with product=True the one product of their Miller values"""
        n = len(g1_aff) // 96
        nt = len(tables_wire) // self.LINE_WIRE_BYTES
        out = C.create_string_buffer(576 * (1 if product else max(n, 1)))
        self._chk(self.lib.nbls_pairing_prepared(self.h, n, g1_aff, tables_wire, nt, int(with_final_exp), int(product), out))
        return out.raw[:576 * (1 if product else n)]

    def g2_prepare_dev(self, n, d_g2, d_tables, stream=None):
        self._chk(self.lib.nbls_g2_prepare_dev(self.h, n, d_g2, d_tables, stream))

    def pairing_prepared_dev(self, n, d_g1, d_tables, d_out, with_final_exp=True, shared_table=False, stream=None):
        self._chk(self.lib.nbls_pairing_prepared_dev(self.h, n, d_g1, d_tables, 0 if shared_table else self.LINE_TABLE_BYTES, int(with_final_exp), d_out, stream))

    def miller_product_prepared_dev(self, n, d_g1, d_tables, d_out, final_exp=True, shared_table=False, stream=None):
        self._chk(self.lib.nbls_miller_product_prepared_dev(self.h, n, d_g1, d_tables, 0 if shared_table else self.LINE_TABLE_BYTES, int(final_exp), d_out, stream))

    def final_exp_batch(self, fp12s):
        n = len(fp12s) // 576
        out = C.create_string_buffer(576 * max(n, 1))
        self._chk(self.lib.nbls_final_exp_batch(self.h, n, fp12s, out))
        return out.raw[:576 * n]

    def validate_batch(self, pts, g2=False):
        sz = 192 if g2 else 96
        n = len(pts) // sz
        st = C.create_string_buffer(max(n, 1))
        self._chk((self.lib.nbls_g2_validate_batch if g2 else self.lib.nbls_g1_validate_batch)(self.h, n, pts, st))
        return list(st.raw[:n])

    def decompress_batch(self, comp, g2=False):
        e = 96 if g2 else 48
        n = len(comp) // e
        out = C.create_string_buffer(max(2 * e * n, 1))
        st = C.create_string_buffer(max(n, 1))
        self._chk((self.lib.nbls_g2_decompress_batch if g2 else self.lib.nbls_g1_decompress_batch)(self.h, n, comp, out, st))
        return out.raw[:2 * e * n], list(st.raw[:n])

    # ---- every wire form of the point codecs (include/nbls.h): kind 'g1' / 'g2' = fromHex, 'sig' = PointG2.fromSignature
    def decode_points(self, kind, blob, length):
        """-> (canonical affine wire bytes, status list); length = bytes per encoded point"""
        n = len(blob) // length
        a = 96 if kind == 'g1' else 192
        out = C.create_string_buffer(max(a * n, 1)); st = C.create_string_buffer(max(n, 1))
        f = {'g1': self.lib.nbls_g1_from_hex_batch, 'g2': self.lib.nbls_g2_from_hex_batch, 'sig': self.lib.nbls_g2_from_signature_batch}[kind]
        self._chk(f(self.h, n, blob, length, out, st))
        return out.raw[:a * n], list(st.raw[:n])

    def encode_points(self, aff, g2=False, compressed=True, zero=None):
        a = 192 if g2 else 96
        n = len(aff) // a
        c = a // 2 if compressed else a
        out = C.create_string_buffer(max(c * n, 1))
        z = bytes(zero) if zero is not None else None
        self._chk((self.lib.nbls_g2_to_hex_batch if g2 else self.lib.nbls_g1_to_hex_batch)(self.h, n, aff, z, int(compressed), out))
        return out.raw[:c * n]

    def clear_cofactor(self, aff, g2=False):
        a = 192 if g2 else 96
        n = len(aff) // a
        out = C.create_string_buffer(max(a * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk((self.lib.nbls_g2_clear_cofactor_batch if g2 else self.lib.nbls_g1_clear_cofactor_batch)(self.h, n, aff, out, st))
        return out.raw[:a * n], list(st.raw[:n])

    @staticmethod
    def _pack(msgs):
        """messages -> (their bytes back to back, uint32 offsets with the end appended) as the C ABI takes them"""
        n = len(msgs)
        if _np is not None and n >= 256:      # 65,536 messages: 6 ms instead of 16 ms of Python loop
            offs = _np.zeros(n + 1, dtype=_np.uint32)
            _np.cumsum(_np.fromiter(map(len, msgs), dtype=_np.uint32, count=n), out=offs[1:])
            return b''.join(msgs), (C.c_uint32 * (n + 1)).from_buffer(offs)
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        return b''.join(msgs), (C.c_uint32 * len(offs))(*offs)

    def hash_to_g2_batch(self, msgs, dst=DST_DEFAULT):
        blob, offs = self._pack(msgs)
        out = C.create_string_buffer(max(192 * len(msgs), 1))
        self._chk(self.lib.nbls_hash_to_g2_batch(self.h, len(msgs), blob, offs, dst, len(dst), out))
        return out.raw[:192 * len(msgs)]

    def hash_to_curve_batch(self, msgs, dst=DST_DEFAULT, g2=False, encode=False):
        """PointG1/PointG2 .hashToCurve (encode=False) or .encodeToCurve (encode=True) -> affine wire bytes"""
        if g2 and not encode:
            return self.hash_to_g2_batch(msgs, dst)
        blob, offs = self._pack(msgs)
        sz = 192 if g2 else 96
        out = C.create_string_buffer(max(sz * len(msgs), 1))
        f = self.lib.nbls_encode_to_g2_batch if g2 else (self.lib.nbls_encode_to_g1_batch if encode else self.lib.nbls_hash_to_g1_batch)
        self._chk(f(self.h, len(msgs), blob, offs, dst, len(dst), out))
        return out.raw[:sz * len(msgs)]

    MAP_UNIFORM_BYTES = {0: (256, 192), 1: (128, 192), 2: (128, 96), 3: (64, 96)}

    def map_uniform_batch(self, kind, uniform):
        """hash-to-curve behind expand_message_xmd on chosen uniform bytes (include/nbls.h nbls_map_uniform_batch): kind 0 G2 hash (256 bytes per item), 1 G2 encode (128),
        2 G1 hash (128), 3 G1 encode (64) -> (affine wire bytes, status bytes: 1 = the zero point, its bytes all-zero)"""
        if kind not in self.MAP_UNIFORM_BYTES:
            raise NblsError('map_uniform_batch: unknown kind %r' % (kind,))
        isz, osz = self.MAP_UNIFORM_BYTES[kind]
        n = len(uniform) // isz
        if len(uniform) != isz * n:
            raise NblsError('map_uniform_batch: %d bytes are not a multiple of %d' % (len(uniform), isz))
        out = C.create_string_buffer(max(osz * n, 1))
        st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_map_uniform_batch(self.h, kind, n, uniform, out, st))
        return out.raw[:osz * n], st.raw[:n]

    def point_sum(self, pts, g2=False):
        sz = 192 if g2 else 96
        out = C.create_string_buffer(sz)
        st = C.create_string_buffer(1)
        self._chk((self.lib.nbls_g2_sum if g2 else self.lib.nbls_g1_sum)(self.h, len(pts) // sz, pts, out, st))
        return out.raw, st.raw[0]

    # ---- secret-scalar side (reference index.ts:738-752); scalars / keys are 32-byte big-endian strings
    P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab

    def point_mul_batch(self, scalars, pts=None, g2=False):
        """[k_i]P_i -> (affine wire bytes, status bytes); pts=None multiplies the G1 generator (PointG1.fromPrivateKey)"""
        n = len(scalars)
        sz = 192 if g2 else 96
        out = C.create_string_buffer(max(sz * n, 1)); st = C.create_string_buffer(max(n, 1))
        f = self.lib.nbls_g2_mul_batch if g2 else self.lib.nbls_g1_mul_batch
        self._chk(f(self.h, n, pts, b''.join(scalars), out, st))
        return out.raw[:sz * n], st.raw[:n]

    def msm(self, pts, scalars, g2=False):
        """sum_i [k_i]P_i (bucket method on the GPU) -> (affine wire bytes, status); status 1 = the sum is the zero point.
        pts: concatenated affine wire points, scalars: list of 32-byte big-endian strings"""
        n = len(scalars)
        sz = 192 if g2 else 96
        assert len(pts) == sz * n
        out = C.create_string_buffer(sz); st = C.c_int8(0)
        f = self.lib.nbls_g2_msm if g2 else self.lib.nbls_g1_msm
        self._chk(f(self.h, n, pts, b''.join(scalars), out, C.byref(st)))
        return out.raw, st.value

    def msm_batch(self, groups_pts, groups_scalars, g2=False):
        """many independent sums in one call (include/nbls.h nbls_g*_msm_batch).  groups_pts: per group its concatenated affine wire points; groups_scalars: per group the list
        of its 32-byte big-endian scalars, or those already concatenated (an empty group is an empty sum) -> (per group the affine wire bytes, per group the status: 1 = the zero point, all-zero bytes); every
        group's result is byte for byte what msm gives for it alone"""
        sz = 192 if g2 else 96
        m = len(groups_scalars)
        ks = [k if isinstance(k, (bytes, bytearray)) else b''.join(k) for k in groups_scalars]
        assert len(groups_pts) == m and all(len(p) * 32 == sz * len(k) for p, k in zip(groups_pts, ks))
        offs = [0]
        for k in ks:
            offs.append(offs[-1] + len(k) // 32)
        out = C.create_string_buffer(max(sz * m, 1)); st = C.create_string_buffer(max(m, 1))
        f = self.lib.nbls_g2_msm_batch if g2 else self.lib.nbls_g1_msm_batch
        self._chk(f(self.h, m, (C.c_uint32 * len(offs))(*offs), b''.join(groups_pts), b''.join(ks), out, st))
        raw = out.raw
        return [raw[sz * g:sz * g + sz] for g in range(m)], list(st.raw[:m])

    def msm_rows(self, pts, rows, g2=False):
        """many scalar vectors against one set of points (nbls_g*_msm_rows).  pts: the concatenated affine wire points; rows: per row the list of one 32-byte scalar per
        point, or the row's scalars already concatenated -> (per row the affine wire bytes, per row the status) as msm_batch"""
        sz = 192 if g2 else 96
        n, m = len(pts) // sz, len(rows)
        ks = b''.join(r if isinstance(r, (bytes, bytearray)) else b''.join(r) for r in rows)
        assert len(pts) == sz * n and len(ks) == 32 * n * m
        out = C.create_string_buffer(max(sz * m, 1)); st = C.create_string_buffer(max(m, 1))
        f = self.lib.nbls_g2_msm_rows if g2 else self.lib.nbls_g1_msm_rows
        self._chk(f(self.h, n, pts, m, ks, out, st))
        raw = out.raw
        return [raw[sz * g:sz * g + sz] for g in range(m)], list(st.raw[:m])

    def msm_dev(self, g2, n, d_pts, d_scalars, nbits, d_out, d_status, stream=0):
        self._chk(self.lib.nbls_msm_dev(self.h, int(bool(g2)), n, d_pts, d_scalars, nbits, d_out, d_status, stream))

    @classmethod
    def compress_g1(cls, aff96):
        """PointG1.toHex(true) of a non-zero affine point (index.ts:359-371)"""
        x = int.from_bytes(aff96[:48], 'big'); y = int.from_bytes(aff96[48:], 'big')
        return (x + ((y * 2) // cls.P_MOD << 381) + (1 << 383)).to_bytes(48, 'big')

    @classmethod
    def compress_g2(cls, aff192):
        """PointG2.toSignature of a non-zero affine point (index.ts:586-602)"""
        x0, x1, y0, y1 = (int.from_bytes(aff192[48 * i:48 * i + 48], 'big') for i in range(4))
        tmp = y1 * 2 if y1 > 0 else y0 * 2
        z1 = x1 + ((tmp // cls.P_MOD) << 381) + (1 << 383)
        return z1.to_bytes(48, 'big') + x0.to_bytes(48, 'big')

    def compress_batch(self, aff, g2=False):
        """PointG1.toHex(true) / PointG2.toSignature for a batch of non-zero affine points, on the GPU"""
        sz = 192 if g2 else 96
        n = len(aff) // sz
        out = C.create_string_buffer(max(n * sz // 2, 1))
        self._chk((self.lib.nbls_g2_compress_batch if g2 else self.lib.nbls_g1_compress_batch)(self.h, n, aff, out))
        return out.raw[:n * sz // 2]

    # ---- the scalar field Fr and threshold recombination (include/nbls.h: nbls_fr_op_batch, nbls_lagrange_at_zero, nbls_g*_combine_shares); not an interface for secrets
    FR_OPS = {'add': 0, 'sub': 1, 'neg': 2, 'mul': 3, 'sqr': 4, 'inv': 5, 'div': 6, 'pow': 7}

    @staticmethod
    def _fr32(v):
        """an Fr element / identifier / exponent as the C ABI takes it: a Python int (0 <= v < 2^256) or 32 bytes big-endian"""
        if isinstance(v, int):
            return v.to_bytes(32, 'big')
        v = bytes(v)
        if len(v) != 32:
            raise NblsError('expected 32 bytes, got %d' % len(v))
        return v

    def fr_op(self, op, a, b=None):
        """Fr elementwise (math.ts:295-386): op = 'add' | 'sub' | 'neg' | 'mul' | 'sqr' | 'inv' | 'div' | 'pow' (or its NBLS_FROP_* number); a, b: lists of ints or 32-byte values,
        b = the second operands or pow's exponents -> (list of 32-byte canonical results, status list: 5 where inv / div meets 0 mod r)"""
        op = self.FR_OPS[op] if isinstance(op, str) else int(op)
        n = len(a)
        if b is not None and len(b) != n:
            raise NblsError('fr_op: %d first and %d second operands' % (n, len(b)))
        out = C.create_string_buffer(max(32 * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_fr_op_batch(self.h, op, n, b''.join(map(self._fr32, a)), None if b is None else b''.join(map(self._fr32, b)), out, st))
        raw = out.raw   # one copy of the buffer, not one per element
        return [raw[32 * i:32 * i + 32] for i in range(n)], list(st.raw[:n])

    def _groups(self, sizes, ids):
        offs = [0]
        for t in sizes:
            offs.append(offs[-1] + t)
        return (C.c_uint32 * len(offs))(*offs), b''.join(self._fr32(x) for g in ids for x in g)

    def lagrange_at_zero(self, groups):
        """groups: a list of identifier lists -> (per group the list of 32-byte coefficients lambda_k = prod_{j != k} x_j / (x_j - x_k), status list: NBLS_ST_BAD_IDS = 20 for a
        group with an identifier that is 0 mod r or two that are equal mod r -- its coefficients are all-zero)"""
        sizes = [len(g) for g in groups]
        offs, ids = self._groups(sizes, groups)
        n = offs[len(sizes)]
        out = C.create_string_buffer(max(32 * n, 1)); st = C.create_string_buffer(max(len(sizes), 1))
        self._chk(self.lib.nbls_lagrange_at_zero(self.h, len(sizes), offs, ids, out, st))
        raw = out.raw
        return [[raw[32 * k:32 * k + 32] for k in range(offs[g], offs[g + 1])] for g in range(len(sizes))], list(st.raw[:len(sizes)])

    def combine_shares(self, groups, g2=True):
        """groups: a list of (ids, shares): t identifiers (ints or 32-byte values) and t compressed shares (96-byte signature shares, or with g2=False 48-byte public-key shares)
        -> (list of compressed combinations sum_k [lambda_k]share_k, status list: 0, 1 = the zero point (0xc0 00..), 3 / 4 = a share that does not decode, 20 = bad identifiers;
        a group with a status >= 2 yields all-zero bytes)"""
        e = 96 if g2 else 48
        for ids, shares in groups:
            if len(ids) != len(shares) or any(len(x) != e for x in shares):
                raise NblsError('combine_shares: every group needs one %d-byte share per identifier' % e)
        offs, ids = self._groups([len(g[0]) for g in groups], [g[0] for g in groups])
        m = len(groups)
        out = C.create_string_buffer(max(e * m, 1)); st = C.create_string_buffer(max(m, 1))
        f = self.lib.nbls_g2_combine_shares if g2 else self.lib.nbls_g1_combine_shares
        self._chk(f(self.h, m, offs, ids, b''.join(bytes(x) for g in groups for x in g[1]), out, st))
        raw = out.raw
        return [raw[e * g:e * g + e] for g in range(m)], list(st.raw[:m])

    def poly_eval(self, groups, g2=False):
        """Share public keys from commitment polynomials (include/nbls.h nbls_g*_poly_eval).  groups: a list of (coefs, ids): the t compressed coefficients A_j = [a_j]G of one
        polynomial, lowest degree first (48-byte G1 points, or with g2=True 96-byte G2 points), and the identifiers to evaluate it at (ints or 32-byte values, any value)
        -> (per group the list of compressed F(x_k) = sum_j [x_k^j]A_j, per group the status list: 0, 1 = the zero point (0xc0 00..), 3 / 4 = the group's first coefficient that
        does not decode, with all-zero bytes)"""
        e = 96 if g2 else 48
        for coefs, ids in groups:
            if not len(coefs) or not len(ids) or any(len(x) != e for x in coefs):
                raise NblsError('poly_eval: every group needs at least one %d-byte coefficient and one identifier' % e)
        coffs, _ = self._groups([len(g[0]) for g in groups], [])
        ioffs, ids = self._groups([len(g[1]) for g in groups], [g[1] for g in groups])
        m, n = len(groups), ioffs[len(groups)]
        out = C.create_string_buffer(max(e * n, 1)); st = C.create_string_buffer(max(n, 1))
        f = self.lib.nbls_g2_poly_eval if g2 else self.lib.nbls_g1_poly_eval
        self._chk(f(self.h, m, coffs, b''.join(bytes(x) for g in groups for x in g[0]), ioffs, ids, out, st))
        raw, sraw = out.raw, st.raw
        return ([[raw[e * k:e * k + e] for k in range(ioffs[g], ioffs[g + 1])] for g in range(m)], [list(sraw[ioffs[g]:ioffs[g + 1]]) for g in range(m)])

    # ---- KZG (include/nbls.h: nbls_fr_eval_roots, nbls_kzg_verify_proofs, nbls_kzg_verify_blobs); field elements must be canonical here (status 21 otherwise)
    def fr_eval_roots(self, log2_n, polys, zs):
        """polys: n polynomials, each the list of its 2^log2_n values on the roots of unity in bit-reversed order (ints or 32-byte values), or their concatenated bytes; zs: n points
        -> (list of 32-byte values p_i(z_i), status list: 21 = an element or the point is >= r, the value is then all-zero)"""
        n = len(zs)
        ev = bytes(polys) if isinstance(polys, (bytes, bytearray, memoryview)) else b''.join(self._fr32(v) for f in polys for v in f)
        if len(ev) != (32 * n) << log2_n:
            raise NblsError('fr_eval_roots: %d points need %d bytes of values, got %d' % (n, (32 * n) << log2_n, len(ev)))
        out = C.create_string_buffer(max(32 * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_fr_eval_roots(self.h, log2_n, n, ev, b''.join(map(self._fr32, zs)), out, st))
        raw = out.raw
        return [raw[32 * i:32 * i + 32] for i in range(n)], list(st.raw[:n])

    @staticmethod
    def _kzg_args(name, n, commitments48, proofs48, tau_g2_96, seed):
        if len(commitments48) != n or len(proofs48) != n or any(len(x) != 48 for x in commitments48) or any(len(x) != 48 for x in proofs48) or len(tau_g2_96) != 96 or \
           (seed is not None and len(seed) != 32):
            raise NblsError('%s: %d items need %d 48-byte commitments and proofs, 96 bytes of [tau]G2 and a seed of 32 bytes or None' % (name, n, n))

    def kzg_verify_proofs(self, commitments48, zs, ys, proofs48, tau_g2_96, seed=None, per_item=True):
        """verify_kzg_proof_batch: n tuples (commitment, z, y, proof) against the setup's compressed [tau]G2 -> (all_ok, status bytes or None).  statuses: 0 ok, 9 not verified,
        3 / 4 the commitment does not decode, 13 / 14 the proof, 21 z or y is >= r; seed: 32 bytes, None = from the OS; per_item=False: the combined check alone (fast reject)"""
        n = len(zs)
        if len(ys) != n:
            raise NblsError('kzg_verify_proofs: %d points and %d values' % (n, len(ys)))
        self._kzg_args('kzg_verify_proofs', n, commitments48, proofs48, tau_g2_96, seed)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_item else None
        self._chk(self.lib.nbls_kzg_verify_proofs(self.h, n, b''.join(commitments48), b''.join(map(self._fr32, zs)), b''.join(map(self._fr32, ys)), b''.join(proofs48), bytes(tau_g2_96),
                                                  seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_item else None)

    def kzg_verify_blobs(self, log2_n, blobs, commitments48, proofs48, tau_g2_96, seed=None, per_item=True):
        """verify_blob_kzg_proof_batch: blobs = n byte strings of 32 << log2_n bytes each (log2_n = 12: the mainnet blob); the challenge is hashed on host threads, the polynomial
        evaluated on the device -> (all_ok, status bytes or None) as kzg_verify_proofs; 21 also for a blob with an element >= r"""
        n = len(blobs)
        if any(len(b) != 32 << log2_n for b in blobs):
            raise NblsError('kzg_verify_blobs: every blob has %d bytes' % (32 << log2_n))
        self._kzg_args('kzg_verify_blobs', n, commitments48, proofs48, tau_g2_96, seed)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_item else None
        self._chk(self.lib.nbls_kzg_verify_blobs(self.h, log2_n, n, b''.join(blobs), b''.join(commitments48), b''.join(proofs48), bytes(tau_g2_96), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_item else None)

    # ---- Groth16 (include/nbls.h: nbls_groth16_*)
    def groth16_vk(self, alpha_g1_48, beta_g2_96, gamma_g2_96, delta_g2_96, ic48):
        """the verifying key's compressed points (ic48: the m + 1 points IC_0 .. IC_m, a list of 48-byte values or their concatenation) -> Groth16Vk, usable from every Engine
        on this device.  Raises KzgSetupError (with the statuses of alpha, beta, gamma, delta, IC_0 .. IC_m) when an entry does not decode or is the zero point"""
        raw = bytes(ic48) if isinstance(ic48, (bytes, bytearray, memoryview)) else b''.join(bytes(x) for x in ic48)
        m = len(raw) // 48 - 1
        if len(raw) % 48 or not 1 <= m <= 1 << 16 or len(alpha_g1_48) != 48 or any(len(x) != 96 for x in (beta_g2_96, gamma_g2_96, delta_g2_96)):
            raise NblsError('groth16_vk: 48 bytes of alpha, 96 bytes each of beta, gamma, delta and the 2 .. 2^16 + 1 points IC_j of 48 bytes each')
        st = C.create_string_buffer(m + 5)
        h = C.c_void_p()
        r = self.lib.nbls_groth16_vk_create(self.h, m, bytes(alpha_g1_48), bytes(beta_g2_96), bytes(gamma_g2_96), bytes(delta_g2_96), raw, st, C.byref(h))
        if r != 0:
            raise KzgSetupError('groth16_vk: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r), r, st.raw)
        return Groth16Vk(self.lib, h)

    def _g16_inputs(self, name, m, inputs):
        """inputs: one row of m field elements (ints or 32-byte values) per proof -> (n, the packed matrix)"""
        if not inputs or any(len(row) != m for row in inputs):
            raise NblsError('%s: one row or more, every row has %d inputs' % (name, m))
        return len(inputs), b''.join(self._fr32(x) for row in inputs for x in row)

    def groth16_verify(self, vk, proofs192, inputs, seed=None, per_item=True):
        """n proofs (192 bytes each: A || B || C compressed) with their rows of public inputs against one key -> (all_ok, status bytes or None).  statuses: 0 ok, 9 not
        verified, 1 / 3 / 4 A is the zero point / does not decode, 11 / 13 / 14 B, 31 / 33 / 34 C, 21 an input is >= r; seed: 32 bytes, None = from the OS; per_item=False:
        the combined check alone (fast reject)"""
        if getattr(vk, 'h', None) is None:
            raise NblsError('groth16_verify: the key is closed')
        n, mat = self._g16_inputs('groth16_verify', vk.inputs, inputs)
        if len(proofs192) != n or any(len(p) != 192 for p in proofs192) or (seed is not None and len(seed) != 32):
            raise NblsError('groth16_verify: %d rows of inputs need %d proofs of 192 bytes and a seed of 32 bytes or None' % (n, n))
        ok = C.c_int(0)
        st = C.create_string_buffer(n) if per_item else None
        self._chk(self.lib.nbls_groth16_verify(self.h, vk.h, n, b''.join(bytes(p) for p in proofs192), mat, seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_item else None)

    def groth16_prepare_inputs(self, vk, inputs):
        """L_i = IC_0 + sum_j [x_ij]IC_j of every row -> (list of 48-byte compressed points, status list: 0, 1 = the zero point (0xc0 00..), 21 = an input is >= r (48 zero
        bytes))"""
        if getattr(vk, 'h', None) is None:
            raise NblsError('groth16_prepare_inputs: the key is closed')
        n, mat = self._g16_inputs('groth16_prepare_inputs', vk.inputs, inputs)
        out, st = C.create_string_buffer(48 * n), C.create_string_buffer(n)
        self._chk(self.lib.nbls_groth16_prepare_inputs(self.h, vk.h, n, mat, out, st))
        raw = out.raw
        return [raw[48 * i:48 * i + 48] for i in range(n)], list(st.raw[:n])

    def groth16_input_sums(self, inputs, weights, pre=None):
        """the folding kernel on caller-chosen weights (< 2^64): rows of m inputs each -> (the m + 1 sums sum w_i, sum w_i x_ij mod r as ints, status list) over the rows with
        pre[i] == 0 and all inputs canonical"""
        m = len(inputs[0]) if inputs else 0
        if not m:
            raise NblsError('groth16_input_sums: one row or more of one input or more')
        n, mat = self._g16_inputs('groth16_input_sums', m, inputs)
        if len(weights) != n or (pre is not None and len(pre) != n):
            raise NblsError('groth16_input_sums: %d rows need %d weights' % (n, n))
        out, st = C.create_string_buffer(32 * (m + 1)), C.create_string_buffer(n)
        self._chk(self.lib.nbls_groth16_input_sums(self.h, n, m, mat, b''.join(self._fr32(w) for w in weights), None if pre is None else bytes(bytearray(int(p) & 0xff for p in pre)), out, st))
        raw = out.raw
        return [int.from_bytes(raw[32 * j:32 * j + 32], 'big') for j in range(m + 1)], list(st.raw[:n])

    # ---- the Groth16 prover (include/nbls.h: nbls_groth16_pk_*, nbls_groth16_prove, nbls_groth16_quotient)
    def groth16_pk(self, log2_n, n_vars, n_public, matrices, alpha_g1_48, beta_g1_48, beta_g2_96, delta_g1_48, delta_g2_96, a_query48, b_g1_query48, b_g2_query96, l_query48,
                   h_query48):
        """matrices: A, B, C, each a list of rows (at most 2^log2_n of them, the same number in all three), a row a list of (column, coefficient) with the coefficient an int
        or 32 bytes; the queries: lists of compressed points or their concatenation (n_vars, n_vars, n_vars, n_vars - n_public - 1, 2^log2_n - 1 of them) -> Groth16Pk.
        Raises KzgSetupError (with the statuses in the order alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, a_query, b_g1_query, b_g2_query, l_query, h_query) when an
        entry does not decode or a zero point stands where none may"""
        join = lambda x: bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else b''.join(bytes(p) for p in x)
        pts = [bytes(alpha_g1_48), bytes(beta_g1_48), bytes(beta_g2_96), bytes(delta_g1_48), bytes(delta_g2_96), join(a_query48), join(b_g1_query48), join(b_g2_query96),
               join(l_query48), join(h_query48)]
        if not 1 <= log2_n <= 21 or len(matrices) != 3 or len({len(m) for m in matrices}) != 1 or len(matrices[0]) > 1 << log2_n or not 0 < n_public < n_vars:
            raise NblsError('groth16_pk: log2_n in 1 .. 21, 0 < n_public < n_vars, three matrices of the same number of rows, at most 2^log2_n')
        n_aux = n_vars - n_public - 1
        if [len(p) for p in pts] != [48, 48, 96, 48, 96, 48 * n_vars, 48 * n_vars, 96 * n_vars, 48 * n_aux, 48 * ((1 << log2_n) - 1)]:
            raise NblsError('groth16_pk: 48 / 96 bytes per fixed point, n_vars points in a_query, b_g1_query and b_g2_query, n_vars - n_public - 1 in l_query, 2^log2_n - 1 in h_query')
        d = Groth16PkDesc(log2_n=log2_n, n_vars=n_vars, n_public=n_public, n_constraints=len(matrices[0]))
        keep = []
        for name, mat in zip('abc', matrices):
            offs, cols, vals = [0], [], []
            for row in mat:
                for col, v in row:
                    cols.append(int(col)); vals.append(self._fr32(v))
                offs.append(len(cols))
            if any(not 0 <= c < 1 << 32 for c in cols):
                raise NblsError('groth16_pk: a column index outside 32 bits')
            bufs = ((C.c_uint32 * len(offs))(*offs), (C.c_uint32 * max(len(cols), 1))(*cols), C.create_string_buffer(b''.join(vals), max(32 * len(vals), 1)))
            keep.append(bufs)
            for f, b in zip(('_rows', '_cols', '_vals32'), bufs):
                setattr(d, name + f, C.cast(b, C.c_void_p))
        for f, p in zip(('alpha_g1_48', 'beta_g1_48', 'beta_g2_96', 'delta_g1_48', 'delta_g2_96', 'a_query48', 'b_g1_query48', 'b_g2_query96', 'l_query48', 'h_query48'), pts):
            b = C.create_string_buffer(p, max(len(p), 1))
            keep.append(b)
            setattr(d, f, C.cast(b, C.c_void_p))
        st = C.create_string_buffer(5 + 3 * n_vars + n_aux + (1 << log2_n) - 1)
        h = C.c_void_p()
        r = self.lib.nbls_groth16_pk_create(self.h, C.byref(d), st, C.byref(h))
        if r != 0:
            raise KzgSetupError('groth16_pk: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r), r, st.raw)
        pk = Groth16Pk(self.lib, h)
        pk.status = st.raw          # 1 marks a masked (zero) query point
        return pk

    def groth16_prove(self, pk, witnesses, rs=None):
        """one proof per witness z = (1, x_1 .. x_m, aux ..) (a list of n_vars ints or 32-byte values) -> (list of 192-byte proofs A || B || C, status list: 0; 21 an
        element of z, r or s is >= r; 24 the witness does not satisfy the constraints or z_0 != 1; 1 A or B is the zero point -- the proof is then 192 zero bytes).
        rs: one (r, s) per witness, or None: drawn from the OS.  The witness and (r, s) are wiped from the engine's buffers before the call returns"""
        if getattr(pk, 'h', None) is None:
            raise NblsError('groth16_prove: the key is closed')
        nv, n = pk.n_vars, len(witnesses)
        if not n or any(len(z) != nv for z in witnesses) or (rs is not None and (len(rs) != n or any(len(p) != 2 for p in rs))):
            raise NblsError('groth16_prove: one witness or more of %d elements each, and one pair (r, s) per witness or None' % nv)
        raw = b''.join(self._fr32(v) for z in witnesses for v in z)
        out, st = C.create_string_buffer(192 * n), C.create_string_buffer(n)
        self._chk(self.lib.nbls_groth16_prove(self.h, pk.h, n, raw, None if rs is None else b''.join(self._fr32(v) for p in rs for v in p), out, st))
        o = out.raw
        return [o[192 * i:192 * i + 192] for i in range(n)], list(st.raw[:n])

    def groth16_pk_wiped(self, pk):
        """for tests: True when the key's secret arrays (the staged witness and (r, s), z, the three vectors and h, the scalar arrays) read back as zeros"""
        if getattr(pk, 'h', None) is None:
            raise NblsError('groth16_pk_wiped: the key is closed')
        w = C.c_int(0)
        self._chk(self.lib.nbls_groth16_pk_wiped(self.h, pk.h, C.byref(w)))
        return bool(w.value)

    def groth16_quotient(self, log2_n, a, b, c):
        """h = (a b - c) / (X^N - 1) for n triples of N = 2^log2_n values in bit-reversed order (lists of rows of ints or 32-byte values, or concatenated bytes) -> (list of
        the N coefficients of every h as ints, status list: 21 = an element is >= r (the row is all-zero), 24 = a_j b_j != c_j somewhere (the row is unspecified))"""
        raws = [bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else b''.join(self._fr32(x) for row in v for x in row) for v in (a, b, c)]
        row = 32 << log2_n
        if not 1 <= log2_n <= 22 or len(raws[0]) % row or len({len(x) for x in raws}) != 1:
            raise NblsError('groth16_quotient: log2_n in 1 .. 22 and three arrays of the same number of rows of %d bytes' % row)
        n = len(raws[0]) // row
        out, st = C.create_string_buffer(max(len(raws[0]), 1)), C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_groth16_quotient(self.h, log2_n, n, raws[0], raws[1], raws[2], out, st))
        o = out.raw
        return [[int.from_bytes(o[row * i + 32 * j:row * i + 32 * j + 32], 'big') for j in range(1 << log2_n)] for i in range(n)], list(st.raw[:n])

    # ---- KZG, the prover's side (include/nbls.h: nbls_kzg_setup_*, nbls_fr_quotient_roots, nbls_kzg_commit_blobs, nbls_kzg_compute_proofs, nbls_kzg_compute_blob_proofs)
    def kzg_setup(self, log2_n, lagrange48):
        """lagrange48: the 2^log2_n compressed points [L_j(tau)]G1 of the setup in bit-reversed order (a list of 48-byte values or their concatenation) -> KzgSetup, usable from
        every Engine on this device.  Raises KzgSetupError (with the per-entry statuses) when an entry does not decode or is the zero point"""
        raw = bytes(lagrange48) if isinstance(lagrange48, (bytes, bytearray, memoryview)) else b''.join(bytes(x) for x in lagrange48)
        if not 1 <= log2_n <= 12 or len(raw) != 48 << log2_n:
            raise NblsError('kzg_setup: log2_n in 1 .. 12 and %d bytes of points, got %d' % (48 << min(max(log2_n, 0), 12), len(raw)))
        st = C.create_string_buffer(1 << log2_n)
        h = C.c_void_p()
        r = self.lib.nbls_kzg_setup_create(self.h, log2_n, raw, st, C.byref(h))
        if r != 0:
            raise KzgSetupError('kzg_setup: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r), r, st.raw)
        return KzgSetup(self.lib, h)

    @staticmethod
    def _kzg_blobs(name, setup, blobs):
        if getattr(setup, 'h', None) is None:
            raise NblsError('%s: the setup is closed' % name)
        size = 32 << setup.log2_n
        if not blobs or any(len(b) != size for b in blobs):
            raise NblsError('%s: one blob or more, every blob has %d bytes' % (name, size))
        return len(blobs), b''.join(bytes(b) for b in blobs)

    def fr_quotient_roots(self, log2_n, polys, zs):
        """the quotient of the opening of every polynomial at its point (arguments as fr_eval_roots) -> (list of 32-byte values y_i, list of the 2^log2_n 32-byte values q_ij per
        polynomial, status list: 21 = an element or the point is >= r, y and the row are then all-zero)"""
        n = len(zs)
        ev = bytes(polys) if isinstance(polys, (bytes, bytearray, memoryview)) else b''.join(self._fr32(v) for f in polys for v in f)
        if len(ev) != (32 * n) << log2_n:
            raise NblsError('fr_quotient_roots: %d points need %d bytes of values, got %d' % (n, (32 * n) << log2_n, len(ev)))
        y = C.create_string_buffer(max(32 * n, 1)); q = C.create_string_buffer(max(len(ev), 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_fr_quotient_roots(self.h, log2_n, n, ev, b''.join(map(self._fr32, zs)), y, q, st))
        yr, qr, row = y.raw, q.raw, 32 << log2_n
        return [yr[32 * i:32 * i + 32] for i in range(n)], [[qr[row * i + 32 * j:row * i + 32 * j + 32] for j in range(1 << log2_n)] for i in range(n)], list(st.raw[:n])

    def kzg_commit_blobs(self, setup, blobs):
        """blob_to_kzg_commitment for n blobs (byte strings of 32 << setup.log2_n bytes) -> (list of 48-byte commitments, status bytes: 21 = an element >= r, the commitment is
        then 48 zero bytes)"""
        n, raw = self._kzg_blobs('kzg_commit_blobs', setup, blobs)
        out = C.create_string_buffer(48 * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_commit_blobs(self.h, setup.h, n, raw, out, st))
        return [out.raw[48 * i:48 * i + 48] for i in range(n)], st.raw[:n]

    def kzg_compute_proofs(self, setup, blobs, zs):
        """compute_kzg_proof for n (blob, z) pairs -> (list of 48-byte proofs, list of 32-byte values y_i = p_i(z_i), status bytes)"""
        n, raw = self._kzg_blobs('kzg_compute_proofs', setup, blobs)
        if len(zs) != n:
            raise NblsError('kzg_compute_proofs: %d blobs and %d points' % (n, len(zs)))
        out = C.create_string_buffer(48 * n); y = C.create_string_buffer(32 * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_compute_proofs(self.h, setup.h, n, raw, b''.join(map(self._fr32, zs)), out, y, st))
        return [out.raw[48 * i:48 * i + 48] for i in range(n)], [y.raw[32 * i:32 * i + 32] for i in range(n)], st.raw[:n]

    def kzg_compute_blob_proofs(self, setup, blobs, commitments48=None):
        """compute_blob_kzg_proof for n blobs -> (list of 48-byte commitments, list of 48-byte proofs, status bytes).  commitments48: the blobs' commitments (only hashed into
        the challenge, not decoded), or None: the call commits first and returns what it computed"""
        n, raw = self._kzg_blobs('kzg_compute_blob_proofs', setup, blobs)
        if commitments48 is not None and (len(commitments48) != n or any(len(c) != 48 for c in commitments48)):
            raise NblsError('kzg_compute_blob_proofs: %d blobs need %d 48-byte commitments' % (n, n))
        cs = C.create_string_buffer(48 * n); out = C.create_string_buffer(48 * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_compute_blob_proofs(self.h, setup.h, n, raw, None if commitments48 is None else b''.join(bytes(c) for c in commitments48), cs, out, st))
        return [cs.raw[48 * i:48 * i + 48] for i in range(n)], [out.raw[48 * i:48 * i + 48] for i in range(n)], st.raw[:n]

    # ---- PeerDAS (include/nbls.h: nbls_fr_ntt, nbls_kzg_compute_cells, nbls_kzg_monomial_*, nbls_kzg_compute_cells_and_proofs)
    def fr_ntt(self, log2_n, polys, to_evals, shifts=None):
        """the transform of n polynomials of 2^log2_n elements each (lists of ints or 32-byte values, or their concatenated bytes): to_evals False: values on the roots in
        bit-reversed order -> coefficients in natural order; True: the way back.  shifts: None, or one shift s per polynomial (the values are then those on s * w_j)
        -> (list of the 2^log2_n 32-byte elements per polynomial, status list: 21 = an element or the shift is >= r, 5 = the shift is 0 mod r; the row is then all-zero)"""
        raw = bytes(polys) if isinstance(polys, (bytes, bytearray, memoryview)) else b''.join(self._fr32(v) for f in polys for v in f)
        row = 32 << log2_n
        if not 1 <= log2_n <= 12 or len(raw) % row or (shifts is not None and len(shifts) * row != len(raw)):
            raise NblsError('fr_ntt: log2_n in 1 .. 12, polynomials of %d bytes each and one shift per polynomial or None' % row)
        n = len(raw) // row
        out = C.create_string_buffer(max(len(raw), 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_fr_ntt(self.h, log2_n, 1 if to_evals else 0, n, raw, None if shifts is None else b''.join(map(self._fr32, shifts)), out, st))
        o = out.raw
        return [[o[row * i + 32 * j:row * i + 32 * j + 32] for j in range(1 << log2_n)] for i in range(n)], list(st.raw[:n])

    def fr_ntt_large(self, log2_n, polys, to_evals, shifts=None):
        """fr_ntt for polynomials of up to 2^24 elements (nbls_fr_ntt_large: global stages in front of tails of 2^12 elements; the same bytes as fr_ntt where both apply).
        polys and shifts as fr_ntt takes them.  Given bytes -> (bytes, status list); given lists -> (list of the 32-byte elements per polynomial, status list)"""
        as_bytes = isinstance(polys, (bytes, bytearray, memoryview))
        raw = bytes(polys) if as_bytes else b''.join(self._fr32(v) for f in polys for v in f)
        row = 32 << log2_n
        if not 1 <= log2_n <= 24 or len(raw) % row:
            raise NblsError('fr_ntt_large: log2_n in 1 .. 24 and polynomials of %d bytes each' % row)
        n = len(raw) // row
        sh = None if shifts is None else bytes(shifts) if isinstance(shifts, (bytes, bytearray, memoryview)) else b''.join(map(self._fr32, shifts))
        if sh is not None and len(sh) != 32 * n:
            raise NblsError('fr_ntt_large: one shift per polynomial or None')
        out = C.create_string_buffer(max(len(raw), 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_fr_ntt_large(self.h, log2_n, 1 if to_evals else 0, n, raw, sh, out, st))
        if as_bytes:
            return out.raw[:len(raw)], list(st.raw[:n])
        o = out.raw
        return [[o[row * i + 32 * j:row * i + 32 * j + 32] for j in range(1 << log2_n)] for i in range(n)], list(st.raw[:n])

    def fr_ntt_dev(self, log2_n, n, d_in, to_evals, d_out, d_shifts=None, d_status=None, stream=None):
        """nbls_fr_ntt_dev on device addresses (ints, e.g. torch.Tensor.data_ptr()): n polynomials of 2^log2_n elements, d_in -> d_out (equal, or disjoint; 16-byte aligned),
        d_shifts: n x 32 bytes or None, d_status: n bytes or None, stream: a hipStream_t as an int (None: the context's).  Asynchronous, ordered on the stream"""
        self._chk(self.lib.nbls_fr_ntt_dev(self.h, log2_n, 1 if to_evals else 0, n, d_in, d_shifts, d_out, d_status, stream))

    def set_ntt_plan(self, tail_bits=None, pass_bits=None):
        """the plan of fr_ntt_large / fr_ntt_dev: the log size of the tails (NBLS_TUNE_NTT_TAIL_BITS = 26; 1 .. 12, 0: the default 12) and the global stages a launch runs at
        most (NBLS_TUNE_NTT_PASS_BITS = 27; 1 .. 9, 0: the default).  The bytes do not depend on either"""
        if tail_bits is not None: self._chk(self.lib.nbls_set_tuning(self.h, 26, int(tail_bits)))
        if pass_bits is not None: self._chk(self.lib.nbls_set_tuning(self.h, 27, int(pass_bits)))

    def kzg_monomial_setup(self, log2_n, monomial48):
        """monomial48: the 2^log2_n compressed points [tau^i]G1 of the setup in natural order (a list of 48-byte values or their concatenation) -> KzgMonomialSetup, usable
        from every Engine on this device.  Raises KzgSetupError (with the per-entry statuses) when an entry does not decode or is the zero point"""
        raw = bytes(monomial48) if isinstance(monomial48, (bytes, bytearray, memoryview)) else b''.join(bytes(x) for x in monomial48)
        if not 1 <= log2_n <= 12 or len(raw) != 48 << log2_n:
            raise NblsError('kzg_monomial_setup: log2_n in 1 .. 12 and %d bytes of points, got %d' % (48 << min(max(log2_n, 0), 12), len(raw)))
        st = C.create_string_buffer(1 << log2_n)
        h = C.c_void_p()
        r = self.lib.nbls_kzg_monomial_create(self.h, log2_n, raw, st, C.byref(h))
        if r != 0:
            raise KzgSetupError('kzg_monomial_setup: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r), r, st.raw)
        return KzgMonomialSetup(self.lib, h)

    @staticmethod
    def _cells_of(raw, n, log2_n, log2_cell):
        cell, per = 32 << log2_cell, 2 << (log2_n - log2_cell)
        return [[raw[cell * (per * i + k):cell * (per * i + k + 1)] for k in range(per)] for i in range(n)]

    def kzg_compute_cells(self, log2_n, log2_cell, blobs):
        """compute_cells for n blobs (byte strings of 32 << log2_n bytes) with 2^log2_cell elements per cell -> (per blob the list of its 2^(log2_n + 1 - log2_cell) cells, bytes
        each; status bytes: 21 = an element >= r, the blob's cells are then all-zero)"""
        size = 32 << log2_n if 1 <= log2_n <= 12 else -1
        if not 0 <= log2_cell <= log2_n or any(len(b) != size for b in blobs):
            raise NblsError('kzg_compute_cells: log2_n in 1 .. 12, log2_cell in 0 .. log2_n, every blob has %d bytes' % size)
        n = len(blobs)
        out = C.create_string_buffer(max(2 * size * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_kzg_compute_cells(self.h, log2_n, log2_cell, n, b''.join(bytes(b) for b in blobs), out, st))
        return self._cells_of(out.raw, n, log2_n, log2_cell), st.raw[:n]

    def kzg_compute_cells_and_proofs(self, setup, log2_cell, blobs):
        """compute_cells_and_kzg_proofs for n blobs against a KzgMonomialSetup -> (cells as kzg_compute_cells, per blob the list of its cells' 48-byte proofs, status bytes:
        21 = an element >= r, the blob's cells are then all-zero and its proofs 48 zero bytes each)"""
        n, raw = self._kzg_blobs('kzg_compute_cells_and_proofs', setup, blobs)
        log2_n = setup.log2_n
        if not 0 <= log2_cell <= log2_n:
            raise NblsError('kzg_compute_cells_and_proofs: log2_cell in 0 .. %d' % log2_n)
        per = 2 << (log2_n - log2_cell)
        out = C.create_string_buffer(2 * len(raw)); pf = C.create_string_buffer(48 * per * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_compute_cells_and_proofs(self.h, setup.h, log2_cell, n, raw, out, pf, st))
        p = pf.raw
        return self._cells_of(out.raw, n, log2_n, log2_cell), [[p[48 * (per * i + k):48 * (per * i + k + 1)] for k in range(per)] for i in range(n)], st.raw[:n]

    def kzg_fk20_setup(self, monomial, log2_cell):
        """the FK20 handle of a KzgMonomialSetup for cells of 2^log2_cell elements (made on the device: one batched MSM) -> KzgFk20Setup"""
        if getattr(monomial, 'h', None) is None:
            raise NblsError('kzg_fk20_setup: the setup is closed')
        if not 0 <= log2_cell <= monomial.log2_n:
            raise NblsError('kzg_fk20_setup: log2_cell in 0 .. %d' % monomial.log2_n)
        h = C.c_void_p()
        self._chk(self.lib.nbls_kzg_fk20_create(self.h, monomial.h, log2_cell, C.byref(h)))
        return KzgFk20Setup(self.lib, h)

    def kzg_compute_cells_and_proofs_fk20(self, fk, blobs):
        """kzg_compute_cells_and_proofs by FK20 against a KzgFk20Setup (which names log2_cell): the same return value, byte for byte"""
        n, raw = self._kzg_blobs('kzg_compute_cells_and_proofs_fk20', fk, blobs)
        log2_n, log2_cell = fk.log2_n, fk.log2_cell
        per = 2 << (log2_n - log2_cell)
        out = C.create_string_buffer(2 * len(raw)); pf = C.create_string_buffer(48 * per * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_compute_cells_and_proofs_fk20(self.h, fk.h, n, raw, out, pf, st))
        p = pf.raw
        return self._cells_of(out.raw, n, log2_n, log2_cell), [[p[48 * (per * i + k):48 * (per * i + k + 1)] for k in range(per)] for i in range(n)], st.raw[:n]

    def kzg_recover_cells_and_proofs_fk20(self, fk, cell_indices, cells):
        """kzg_recover_cells_and_proofs by FK20 against a KzgFk20Setup: the same return value, byte for byte"""
        if getattr(fk, 'h', None) is None:
            raise NblsError('kzg_recover_cells_and_proofs_fk20: the setup is closed')
        log2_n, log2_cell, n = fk.log2_n, fk.log2_cell, len(cells)
        off, idx, raw = self._recover_args('kzg_recover_cells_and_proofs_fk20', log2_n, log2_cell, cell_indices, cells)
        if not n:
            raise NblsError('kzg_recover_cells_and_proofs_fk20: one blob or more')
        per = 2 << (log2_n - log2_cell)
        out = C.create_string_buffer((64 << log2_n) * n); pf = C.create_string_buffer(48 * per * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_recover_cells_and_proofs_fk20(self.h, fk.h, n, off, idx, raw, out, pf, st))
        p = pf.raw
        return self._cells_of(out.raw, n, log2_n, log2_cell), [[p[48 * (per * i + k):48 * (per * i + k + 1)] for k in range(per)] for i in range(n)], st.raw[:n]

    def _recover_args(self, name, log2_n, log2_cell, cell_indices, cells):
        size = 32 << log2_cell if 0 <= log2_cell <= log2_n else -1
        if not 1 <= log2_n <= 12 or size < 0 or len(cell_indices) != len(cells) or any(len(i) != len(c) for i, c in zip(cell_indices, cells)) or \
           any(not 0 <= int(k) < 1 << 32 for i in cell_indices for k in i) or any(len(x) != size for c in cells for x in c) or sum(len(i) for i in cell_indices) >= 1 << 32:
            raise NblsError('%s: log2_n in 1 .. 12, log2_cell in 0 .. log2_n, per blob a list of cell indices and as many cells of %d bytes each' % (name, size))
        off = [0]
        for i in cell_indices:
            off.append(off[-1] + len(i))
        flat = [int(k) for i in cell_indices for k in i]
        return (C.c_uint32 * len(off))(*off), (C.c_uint32 * len(flat))(*flat) if flat else None, b''.join(bytes(x) for c in cells for x in c) if flat else None

    def kzg_recover_cells(self, log2_n, log2_cell, cell_indices, cells):
        """recover_cells for n blobs from at least half of each blob's cells: cell_indices[i] lists the cell numbers given for blob i (any order), cells[i] those cells (byte
        strings of 32 << log2_cell bytes, as kzg_compute_cells returns them) -> (per blob the list of ALL its cells, as kzg_compute_cells; status bytes: 22 = fewer than half of
        the cells, an index out of range or twice, 21 = an element >= r, 23 = the given cells contradict one another; the blob's cells are then all-zero)"""
        off, idx, raw = self._recover_args('kzg_recover_cells', log2_n, log2_cell, cell_indices, cells)
        n = len(cells)
        out = C.create_string_buffer(max((64 << log2_n) * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_kzg_recover_cells(self.h, log2_n, log2_cell, n, off, idx, raw, out, st))
        return self._cells_of(out.raw, n, log2_n, log2_cell), st.raw[:n]

    def kzg_recover_cells_and_proofs(self, monomial, log2_cell, cell_indices, cells):
        """recover_cells_and_kzg_proofs against a KzgMonomialSetup: the arguments of kzg_recover_cells -> (cells, proofs, status bytes) as kzg_compute_cells_and_proofs returns
        them for the recovered blobs; a refused blob (statuses as kzg_recover_cells) has all-zero cells and 48 zero bytes for every proof"""
        if getattr(monomial, 'h', None) is None:
            raise NblsError('kzg_recover_cells_and_proofs: the setup is closed')
        log2_n, n = monomial.log2_n, len(cells)
        off, idx, raw = self._recover_args('kzg_recover_cells_and_proofs', log2_n, log2_cell, cell_indices, cells)
        if not n:
            raise NblsError('kzg_recover_cells_and_proofs: one blob or more')
        per = 2 << (log2_n - log2_cell)
        out = C.create_string_buffer((64 << log2_n) * n); pf = C.create_string_buffer(48 * per * n); st = C.create_string_buffer(n)
        self._chk(self.lib.nbls_kzg_recover_cells_and_proofs(self.h, monomial.h, log2_cell, n, off, idx, raw, out, pf, st))
        p = pf.raw
        return self._cells_of(out.raw, n, log2_n, log2_cell), [[p[48 * (per * i + k):48 * (per * i + k + 1)] for k in range(per)] for i in range(n)], st.raw[:n]

    def kzg_verify_cells(self, monomial, log2_cell, commitments48, commitment_index, cell_index, cells, proofs48, tau_c_g2_96, seed=None, per_item=True):
        """verify_cell_kzg_proof_batch against a KzgMonomialSetup: cell k of the call is cell number cell_index[k] of the blob with commitment commitments48[commitment_index[k]]
        (every commitment once; cells may repeat); cells: byte strings of 32 << log2_cell bytes (log2_cell <= 6), as kzg_compute_cells returns them; tau_c_g2_96: the setup's
        compressed [tau^c]G2 -> (all_ok, status bytes or None).  statuses: 0 ok, 9 not verified, 3 / 4 the commitment does not decode, 13 / 14 the proof, 21 an element is >= r;
        seed: 32 bytes, None = from the OS; per_item=False: the combined check alone (fast reject)"""
        if getattr(monomial, 'h', None) is None:
            raise NblsError('kzg_verify_cells: the setup is closed')
        n, size = len(cells), 32 << log2_cell if 0 <= log2_cell <= 6 else -1
        if not n or not commitments48 or len(commitment_index) != n or len(cell_index) != n or len(proofs48) != n or any(len(x) != size for x in cells) or \
           any(len(x) != 48 for x in commitments48) or any(len(x) != 48 for x in proofs48) or len(tau_c_g2_96) != 96 or (seed is not None and len(seed) != 32) or \
           any(not 0 <= int(i) < 1 << 32 for i in commitment_index) or any(not 0 <= int(i) < 1 << 32 for i in cell_index):
            raise NblsError('kzg_verify_cells: one cell or more of %d bytes each (log2_cell in 0 .. 6), with an index into the 48-byte commitments, a cell index and a 48-byte proof '
                            'each, 96 bytes of [tau^c]G2 and a seed of 32 bytes or None' % size)
        ok = C.c_int(0)
        st = C.create_string_buffer(n) if per_item else None
        u32s = C.c_uint32 * n
        self._chk(self.lib.nbls_kzg_verify_cells(self.h, monomial.h, log2_cell, len(commitments48), b''.join(bytes(x) for x in commitments48), n, u32s(*commitment_index), u32s(*cell_index),
                                                 b''.join(bytes(x) for x in cells), b''.join(bytes(x) for x in proofs48), bytes(tau_c_g2_96), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_item else None)

    def get_public_keys(self, keys):
        """getPublicKey for a batch of private keys -> list of 48-byte compressed keys; raises like the reference on a zero key"""
        aff, st = self.point_mul_batch(keys)
        if any(st):
            raise NblsError('Private key must be 0 < key < CURVE.r')
        c = self.compress_batch(aff)
        return [c[48 * i:48 * i + 48] for i in range(len(keys))]

    def sign_batch_affine(self, msgs, keys, dst=DST_DEFAULT):
        """nbls_sign_batch as is: (n * 192 affine signature bytes, status bytes)"""
        blob, offs = self._pack(msgs)
        n = len(msgs)
        out = C.create_string_buffer(max(192 * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_sign_batch(self.h, n, blob, offs, dst, len(dst), b''.join(keys), out, st))
        return out.raw[:192 * n], st.raw[:n]

    def sign_batch_dev(self, n, d_msgs, d_offsets, d_keys32, d_out192, d_status, dst=DST_DEFAULT, stream=None):
        """nbls_sign_batch_dev: everything resident in device memory (pointers as integers); synchronises"""
        self._chk(self.lib.nbls_sign_batch_dev(self.h, n, C.c_void_p(d_msgs), C.c_void_p(d_offsets), dst, len(dst), C.c_void_p(d_keys32), C.c_void_p(d_out192), C.c_void_p(d_status), stream))

    def sign_packed(self, n, blob, offs, keys_blob, out, st, dst=DST_DEFAULT):
        """nbls_sign_batch on buffers the caller has already packed (message bytes, ctypes uint32 offsets, n * 32 key bytes) into preallocated ctypes outputs: the C-ABI call by itself"""
        self._chk(self.lib.nbls_sign_batch(self.h, n, blob, offs, dst, len(dst), keys_blob, out, st))

    def sign_batch(self, msgs, keys, dst=DST_DEFAULT):
        """sign(msg_i, key_i) -> list of 96-byte compressed signatures"""
        aff, st = self.sign_batch_affine(msgs, keys, dst)
        if any(st):
            raise NblsError('Private key must be 0 < key < CURVE.r')
        c = self.compress_batch(aff, g2=True)
        return [c[96 * i:96 * i + 96] for i in range(len(msgs))]

    def verify_batch(self, sig96, msgs, pks48, dst=DST_DEFAULT):
        """-> True/False; raises NblsError where the reference throws while decoding its arguments"""
        blob, offs = self._pack(msgs)
        ok = C.c_int(0)
        self._chk(self.lib.nbls_verify_batch(self.h, len(msgs), sig96, blob, offs, b''.join(pks48), dst, len(dst), C.byref(ok)))
        return bool(ok.value)

    def verify_multiple(self, sigs96, msgs, pks48, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify(sig_i, msg_i, pk_i) for n independent sets, checked together by a random linear combination (nbls_verify_multiple) -> (all_ok, statuses or None).
        statuses: bytes, one per set (0 ok, 9 not verified, the key's decoder status, 10 + the signature's, 1 / 11 for a zero key / signature); seed: 32 bytes, None = from the OS;
        per_set=False: the combined check alone (fast reject, statuses None)"""
        n = len(msgs)
        if len(sigs96) != n or len(pks48) != n or (seed is not None and len(seed) != 32):
            raise NblsError('verify_multiple: %d messages, %d signatures, %d keys, seed of %s bytes' % (n, len(sigs96), len(pks48), None if seed is None else len(seed)))
        blob, offs = self._pack(msgs)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_multiple(self.h, n, b''.join(sigs96), blob, offs, b''.join(pks48), dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    @staticmethod
    def _u32(vals):
        """a sequence of non-negative ints -> a ctypes uint32 array"""
        n = len(vals)
        if _np is not None and n >= 256:
            return (C.c_uint32 * n).from_buffer(_np.ascontiguousarray(vals, dtype=_np.uint32))
        return (C.c_uint32 * n)(*vals)

    def _key_offsets(self, sets):
        lens = [len(k) for k in sets]
        if _np is not None and len(lens) >= 256:
            offs = _np.zeros(len(lens) + 1, dtype=_np.uint32)
            _np.cumsum(_np.fromiter(lens, dtype=_np.uint32, count=len(lens)), out=offs[1:])
            return (C.c_uint32 * len(offs)).from_buffer(offs)
        offs = [0]
        for k in lens:
            offs.append(offs[-1] + k)
        return (C.c_uint32 * len(offs))(*offs)

    def verify_aggregates(self, sigs96, msgs, key_sets, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify(sig_j, msg_j, aggregatePublicKeys(key_sets[j])) for n sets, checked together by a random linear combination (nbls_verify_aggregates) -> (all_ok, statuses or None).
        key_sets: a list of lists of 48-byte compressed keys.  statuses: bytes, one per set (0 ok, 9 not verified, the first bad key's decoder status, 10 + the signature's,
        1 when the keys sum to zero, 11 for a zero signature); seed and per_set as verify_multiple"""
        n = len(msgs)
        if len(sigs96) != n or len(key_sets) != n or (seed is not None and len(seed) != 32):
            raise NblsError('verify_aggregates: %d messages, %d signatures, %d key sets, seed of %s bytes' % (n, len(sigs96), len(key_sets), None if seed is None else len(seed)))
        blob, offs = self._pack(msgs)
        koffs = self._key_offsets(key_sets)
        pks = b''.join(b''.join(k) for k in key_sets)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_aggregates(self.h, n, b''.join(sigs96), blob, offs, pks, koffs, dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    def create_keyset(self, pks48):
        """nbls_keyset_create: decode the keys once into a table in this device's memory -> (KeySet, status bytes: 0, 1 for the zero key, 3, 4 per key)"""
        n = len(pks48)
        h = C.c_void_p()
        st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_keyset_create(self.h, n, b''.join(pks48), st, C.byref(h)))
        return KeySet(self.lib, h), st.raw[:n]

    def verify_aggregates_indexed(self, keyset, sigs96, msgs, index_sets, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify_aggregates with the keys of set j named by their indices in `keyset` (a KeySet of create_keyset): index_sets is a list of lists of ints"""
        n = len(msgs)
        if len(sigs96) != n or len(index_sets) != n or (seed is not None and len(seed) != 32):
            raise NblsError('verify_aggregates_indexed: %d messages, %d signatures, %d index sets, seed of %s bytes' % (n, len(sigs96), len(index_sets), None if seed is None else len(seed)))
        if keyset.h is None:
            raise NblsError('verify_aggregates_indexed: the key table is closed')
        blob, offs = self._pack(msgs)
        koffs = self._key_offsets(index_sets)
        idx = self._u32([i for s in index_sets for i in s])
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_aggregates_indexed(self.h, keyset.h, n, b''.join(sigs96), blob, offs, idx, koffs, dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    def _shared_args(self, what, sigs96, msgs, msg_index, sets, seed):
        """-> n, the packed messages, their offsets and the message index as a ctypes uint32 array.  A numpy uint32 array is taken as it is (no copy); a list of 65,536 ints
        costs ~3 ms to check and convert, a tenth of the call"""
        n = len(sigs96)
        if len(msg_index) != n or len(sets) != n or (seed is not None and len(seed) != 32):
            raise NblsError('%s: %d signatures, %d message indices, %d keys or key sets, seed of %s bytes' % (what, n, len(msg_index), len(sets), None if seed is None else len(seed)))
        if _np is not None and isinstance(msg_index, _np.ndarray) and msg_index.dtype == _np.uint32 and msg_index.ndim == 1:
            a = _np.ascontiguousarray(msg_index)
            idx = (C.c_uint32 * n).from_buffer(a if a.flags.writeable else a.copy())
        else:
            if n and not 0 <= min(msg_index) <= max(msg_index) <= 0xffffffff:
                raise NblsError('%s: a message index outside 0 .. 2^32 - 1' % what)
            idx = self._u32(msg_index)
        blob, offs = self._pack(msgs)
        return n, blob, offs, idx

    def verify_multiple_shared(self, sigs96, msgs, msg_index, pks48, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify_multiple for sets that share messages (nbls_verify_multiple_shared): msgs holds the distinct messages, set i signs msgs[msg_index[i]]; one hash and one Miller
        loop per message.  Returns what verify_multiple returns for the expanded input and the same seed.  group_messages turns a flat list into (msgs, msg_index)"""
        n, blob, offs, idx = self._shared_args('verify_multiple_shared', sigs96, msgs, msg_index, pks48, seed)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_multiple_shared(self.h, n, b''.join(sigs96), len(msgs), blob, offs, idx, b''.join(pks48), dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    def verify_aggregates_shared(self, sigs96, msgs, msg_index, key_sets, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify_aggregates for sets that share messages (nbls_verify_aggregates_shared): msgs and msg_index as verify_multiple_shared"""
        n, blob, offs, idx = self._shared_args('verify_aggregates_shared', sigs96, msgs, msg_index, key_sets, seed)
        koffs = self._key_offsets(key_sets)
        pks = b''.join(b''.join(k) for k in key_sets)
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_aggregates_shared(self.h, n, b''.join(sigs96), len(msgs), blob, offs, idx, pks, koffs, dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    def verify_aggregates_indexed_shared(self, keyset, sigs96, msgs, msg_index, index_sets, dst=DST_DEFAULT, seed=None, per_set=True):
        """verify_aggregates_indexed for sets that share messages (nbls_verify_aggregates_indexed_shared): msgs and msg_index as verify_multiple_shared"""
        n, blob, offs, idx = self._shared_args('verify_aggregates_indexed_shared', sigs96, msgs, msg_index, index_sets, seed)
        if keyset.h is None:
            raise NblsError('verify_aggregates_indexed_shared: the key table is closed')
        koffs = self._key_offsets(index_sets)
        kidx = self._u32([i for s in index_sets for i in s])
        ok = C.c_int(0)
        st = C.create_string_buffer(max(n, 1)) if per_set else None
        self._chk(self.lib.nbls_verify_aggregates_indexed_shared(self.h, keyset.h, n, b''.join(sigs96), len(msgs), blob, offs, idx, kidx, koffs, dst, len(dst), seed, C.byref(ok), st))
        return bool(ok.value), (st.raw[:n] if per_set else None)

    def verify_batch_dev(self, n, d_sig, d_uniform, d_pk, stream=None):
        ok = C.c_int(0)
        self._chk(self.lib.nbls_verify_batch_dev_inputs(self.h, n, d_sig, d_uniform, d_pk, C.byref(ok), None, stream))
        return bool(ok.value)

    def verify_batch_msgs_dev(self, n, d_sig, d_msgs, d_offsets, d_pk, dst=DST_DEFAULT, stream=None):
        """verifyBatch with signature, message bytes + uint32 offsets and compressed keys resident in HBM: expand_message_xmd runs on the device as part of the call"""
        ok = C.c_int32(0)
        self._chk(self.lib.nbls_verify_batch_msgs_dev(self.h, n, d_sig, d_msgs, d_offsets, d_pk, dst, len(dst), C.byref(ok), stream))
        return bool(ok.value)

    def verify_batch_partial_dev(self, n, d_sig, d_uniform, d_pk, d_out, stream=None):
        """one rank's share of a multi-GPU verifyBatch: Miller product of its n pairs (plus (-G, S) when d_sig is not None/0) without
        the final exponentiation -> 576 wire bytes at d_out; returns True when a zero point was met (the batch verifies false)"""
        z = C.c_int(0)
        self._chk(self.lib.nbls_verify_batch_partial_dev(self.h, n, d_sig or None, d_uniform, d_pk, d_out, C.byref(z), None, stream))
        return bool(z.value)

    # ---- device-pointer entry points (torch uint8 CUDA tensors); enqueue on `stream` (int handle) or the context stream
    def pairing_batch_dev(self, n, d_g1, d_g2, d_out, with_final_exp=True, stream=None):
        self._chk(self.lib.nbls_pairing_batch_dev(self.h, n, d_g1, d_g2, int(with_final_exp), d_out, stream))

    def miller_product_dev(self, n, d_g1, d_g2, d_out, final_exp=True, stream=None):
        self._chk(self.lib.nbls_miller_product_dev(self.h, n, d_g1, d_g2, int(final_exp), d_out, stream))

    def final_exp_batch_dev(self, n, d_in, d_out, stream=None):
        self._chk(self.lib.nbls_final_exp_batch_dev(self.h, n, d_in, d_out, stream))

    def fp12_product_final_dev(self, n, d_in, d_out, final_exp=True, stream=None):
        self._chk(self.lib.nbls_fp12_product_final_dev(self.h, n, d_in, int(final_exp), d_out, stream))

    def set_expc_min(self, n):
        """items from which the final exponentiation uses compressed cyclotomic squarings (NBLS_TUNE_EXPC_MIN; 0 = always)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 3, n))

    def set_split_miller_min(self, n):
        """pairs from which the Miller loop runs as LINES + ACC (0: always, a huge value: never)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 1, n))

    def set_halves_min(self, n):
        """pairs from which pairing_batch_dev runs a batch as two halves on two streams (default 16384; 0: never)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 2, n))

    def set_chain_max(self, n):
        """items below which the middle of the final exponentiation is one chained launch (NBLS_TUNE_CHAIN_MAX; default 8192, 0: one launch per program)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 4, n))

    def set_fe_tail_chain(self, bits):
        """which short programs of a final exponentiation that runs launch by launch end inside the exponentiation's launch before them (NBLS_TUNE_FE_TAIL_CHAIN): bit 0 the
        final product, bit 1 FE_MID1 / FE_MID2; default 0, pool contexts are set by nbls_pool_init"""
        self._chk(self.lib.nbls_set_tuning(self.h, 24, int(bits)))

    def set_fe_head_chain(self, on):
        """such a final exponentiation runs the easy part at the head of the first exponentiation's launch (NBLS_TUNE_FE_HEAD_CHAIN): 0 / 1; default 0, pool contexts are set by
        nbls_pool_init"""
        self._chk(self.lib.nbls_set_tuning(self.h, 29, int(on)))

    def set_inv_prio(self, level):
        """issue priority 0 .. 3 of the wavefronts of the one-element-per-lane Fp inversion kernel (NBLS_TUNE_INV_PRIO); default 0, pool contexts are set by nbls_pool_init"""
        self._chk(self.lib.nbls_set_tuning(self.h, 30, int(level)))

    def set_sac_max(self, n):
        """keys up to which sign's ladder is the sign-aligned one-addition-per-bit form (NBLS_TUNE_SAC_MAX; default 6144, 0: the windowed psi-split ladder at every size)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 8, n))

    def set_wide_max(self, n):
        """items up to which the programs that allow it run on the one-limb-per-lane interpreter (NBLS_TUNE_WIDE_MAX; an experiment, measured slower than the lane-split forms: default 0 = never)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 10, n))

    def set_ls_max(self, ls_max=None, ls2_max=None):
        """items up to which the pairing programs run in their four-lane / two-lane forms (NBLS_TUNE_LS_MAX = 13, NBLS_TUNE_LS2_MAX = 14; defaults 1024 / 2048, pool contexts 0 / 0)"""
        if ls_max is not None: self._chk(self.lib.nbls_set_tuning(self.h, 13, int(ls_max)))
        if ls2_max is not None: self._chk(self.lib.nbls_set_tuning(self.h, 14, int(ls2_max)))

    def set_inv_wide_max(self, n):
        """elements up to which an Fp inversion launch runs with one limb per lane (NBLS_TUNE_INV_WIDE_MAX = 12; default 4096, pool contexts 256, 0: never)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 12, int(n)))

    def set_h2c_norm_min(self, n):
        """messages from which hash-to-G2 takes its SWU square root by the norm method (NBLS_TUNE_H2C_NORM_MIN = 11; default 32768, 0: always)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 11, int(n)))

    def set_pt_ls2_max(self, n):
        """items up to which the G2 point chains of verify / sign run in their two-lane forms (NBLS_TUNE_PT_LS2_MAX; default 4096, 0: never)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 9, n))

    def set_poly_slab(self, n):
        """identifiers that poly_eval works through at a time (NBLS_TUNE_POLY_SLAB = 15; default 2^18, 0: the default)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 15, int(n)))

    def set_msm_batch(self, window=None, big=None, slab=None):
        """msm_batch / msm_rows (NBLS_TUNE_MSMB_WINDOW = 16 / _BIG = 17 / _SLAB = 18): the window width (4, 6, 8, 10, 12; 0: chosen per call), the points above which a group
        runs alone through the pipeline of msm, the budget of a slab of groups; 0: the defaults"""
        for key, v in ((16, window), (17, big), (18, slab)):
            if v is not None:
                self._chk(self.lib.nbls_set_tuning(self.h, key, int(v)))

    def set_cells_chunk(self, blobs):
        """blobs that kzg_compute_cells_and_proofs hands to the batched MSM in one pass (NBLS_TUNE_CELLS_CHUNK = 20; 0: as many as its bounds take)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 20, int(blobs)))

    def set_groth16_chunk(self, proofs):
        """proofs that the per-proof pass of groth16_verify and groth16_prepare_inputs hand to the batched MSM in one pass (NBLS_TUNE_G16_CHUNK = 22; 0: as many as its bounds take)"""
        self._chk(self.lib.nbls_set_tuning(self.h, 22, int(proofs)))

    def set_groth16_row_wave(self, entries):
        """matrix entries from which groth16_prove sums a row by a whole wavefront instead of one lane (NBLS_TUNE_G16P_ROW_WAVE = 31; 0: the default).  The bytes do not depend on it"""
        self._chk(self.lib.nbls_set_tuning(self.h, 31, int(entries)))

    def set_verify_pipeline(self, chunks=None, last_pct=None, pipe_min=None):
        """verifyBatch as a software pipeline (NBLS_TUNE_VERIFY_CHUNKS / _LAST_PCT / _PIPE_MIN): number of chunks (0 / 1: one), size of the last chunk in
        per cent of the batch, signatures from which a call is chunked at all"""
        for key, v in ((5, chunks), (6, last_pct), (7, pipe_min)):
            if v is not None:
                self._chk(self.lib.nbls_set_tuning(self.h, key, v))

    def synchronize(self):
        self._chk(self.lib.nbls_device_synchronize(self.h))

    def program_stats(self, name):
        o = (C.c_uint32 * 8)()
        self._chk(self.lib.nbls_program_stats(self.h, PROGRAMS.index(name), o))
        keys = ['steps', 'dot_steps', 'lin_steps', 'dot_ops', 'products', 'lin_ops', 'slots', 'lds_bytes']
        return dict(zip(keys, list(o)))

    def program_kernel(self, name):
        """the kernel that executes step program `name` in this context: 'nbls_aot_<kernel>' or 'nbls_vm_kernel[_ls4]' (the interpreter)"""
        k = self.lib.nbls_program_kernel(self.h, PROGRAMS.index(name))
        if k is None:
            raise NblsError('nbls_program_kernel(%s) failed' % name)
        return k.decode()

    def extra_program_kernel(self, name):
        """the same for a program outside PROGRAMS, by name: 'poly_g1_16', 'poly_g1_256', 'poly_g2_16', 'poly_g2_256' (the Horner steps of poly_eval), 'dbladd_g1', 'dbladd_g2'
        (the combination steps of msm_batch / msm_rows), 'lines_fe' (the line program of the pairings that end in a final exponentiation)"""
        k = self.lib.nbls_extra_program_kernel(self.h, name.encode())
        if k is None:
            raise NblsError('nbls_extra_program_kernel(%s) failed' % name)
        return k.decode()

    def extra_program_launches(self, name):
        """launches of a program outside PROGRAMS in this context so far (they are booked in the timing slot of the stage they serve: 'lines_fe' in 'lines_pq')"""
        self.lib.nbls_extra_program_launches.restype = C.c_longlong
        self.lib.nbls_extra_program_launches.argtypes = [C.c_void_p, C.c_char_p]
        return self.lib.nbls_extra_program_launches(self.h, name.encode())

    def chain_launches(self):
        """launches of this context so far that ran several programs as one launch (nbls_chain_launches; a chain's fallback of one launch per program does not count)"""
        self.lib.nbls_chain_launches.restype = C.c_longlong
        self.lib.nbls_chain_launches.argtypes = [C.c_void_p]
        return self.lib.nbls_chain_launches(self.h)

    def kernel_bindings(self):
        """{program: kernel} over every step program"""
        return {p: self.program_kernel(p) for p in PROGRAMS}

    def device_synchronize(self):
        self._chk(self.lib.nbls_device_synchronize(self.h))

    def timing_enable(self, on=True):
        self._chk(self.lib.nbls_timing_enable(self.h, int(on)))

    def tower_op(self, field, op, a, b=None, c=None, d=None, param=0):
        """one tower operation (include/nbls.h NBLS_TOP_*) on len(a) / (48 * field) elements given as wire bytes -> wire bytes"""
        esz = 48 * field
        n = len(a) // esz
        out = C.create_string_buffer(n * esz)
        args = [C.c_char_p(x) if x is not None else None for x in (a, b, c, d)]
        self._chk(self.lib.nbls_tower_op_batch(self.h, C.c_int(field), C.c_int(op), C.c_int(param), C.c_size_t(n), args[0], args[1], args[2], args[3], out))
        return out.raw

    FIELD_KINDS = {'sqrt': 0, 'fp2_sqrt': 1, 'fp2_sqrt_div': 2, 'swu': 3, 'inv': 4}

    def field_kernel_raw(self, kind, form, n, raw, out=None):
        """the stand-alone field kernels on raw scratch elements (include/nbls.h nbls_field_kernel_raw): kind = 0 .. 3 (the exponents (p+1)/4, (p^2+7)/16, (p^2-9)/16, (p-3)/4)
        or 4 (the Montgomery inverse), or its name in FIELD_KINDS; form = 1 (one element per lane), 2 (one limb per lane) or 0 (what the pipelines would take for this n);
        raw: n elements of 64 bytes (kinds 1, 2: 2 n, c0 then c1); out: a ctypes buffer to write into (it may be longer: the call writes the elements' bytes only) -> its bytes"""
        kind = self.FIELD_KINDS[kind] if isinstance(kind, str) else int(kind)
        size = 64 * n * (2 if kind in (1, 2) else 1)
        if len(raw) < size:
            raise NblsError('field_kernel_raw: %d bytes for %d elements' % (len(raw), n))
        if out is None:
            out = C.create_string_buffer(max(size, 1))
        elif len(out) < size:
            raise NblsError('field_kernel_raw: output buffer of %d bytes for %d elements' % (len(out), n))
        self._chk(self.lib.nbls_field_kernel_raw(self.h, kind, int(form), n, raw, out))
        return out.raw

    def config_describe(self):
        """the environment switches the library has read so far, with the values in force"""
        return self.lib.nbls_config_describe().decode()

    def timing_read(self):
        """-> {kernel name: (total ms, launches)} since timing_enable(True)"""
        n = len(PROGRAMS) + 1
        ms = (C.c_float * n)()
        cnt = (C.c_uint32 * n)()
        self._chk(self.lib.nbls_timing_read(self.h, ms, cnt))
        names = PROGRAMS + ['fp_inv']
        return {names[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i]}


class MultiEngine:
    """Several GPUs of one node behind one handle (include/nbls.h nbls_init_multi): contiguous shards, one host thread and stream per
    device, 576-byte Fp12 partials gathered on the first device by hipMemcpyPeer.  devices=None takes every visible device; a device id
    may be listed more than once (several contexts on one GPU: the tests exercise the sharded paths on a one-GPU box that way)."""

    def __init__(self, devices=None):
        self.lib = load_library()
        h = C.c_void_p()
        if devices is None:
            r = self.lib.nbls_init_multi(0, None, C.byref(h))
        else:
            ids = (C.c_int * len(devices))(*devices)
            r = self.lib.nbls_init_multi(len(devices), ids, C.byref(h))
        if r != 0:
            raise NblsError('nbls_init_multi failed: %s (code %d)' % (self.lib.nbls_strerror(r).decode(), r))
        self.h = h
        self.n_devices = self.lib.nbls_multi_device_count(h)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.nbls_destroy_multi(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != 0:
            raise NblsError('%s (code %d)' % (self.lib.nbls_strerror(r).decode(), r))

    def pairing_batch(self, g1_aff, g2_aff, with_final_exp=True, validate=False):
        n = len(g1_aff) // 96
        out = C.create_string_buffer(max(576 * n, 1)); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_multi_pairing_batch(self.h, n, g1_aff, g2_aff, int(with_final_exp), int(validate), out, st))
        return out.raw[:576 * n], st.raw[:n]

    def miller_product(self, g1_aff, g2_aff, final_exp=True, validate=False):
        n = len(g1_aff) // 96
        out = C.create_string_buffer(576); st = C.create_string_buffer(max(n, 1))
        self._chk(self.lib.nbls_multi_miller_product(self.h, n, g1_aff, g2_aff, int(final_exp), int(validate), out, st))
        return out.raw, st.raw[:n]

    def verify_batch(self, sig96, msgs, pks48, dst=DST_DEFAULT):
        blob, offs = Engine._pack(msgs)
        ok = C.c_int(0)
        self._chk(self.lib.nbls_multi_verify_batch(self.h, len(msgs), sig96, blob, offs, b''.join(pks48), dst, len(dst), C.byref(ok)))
        return bool(ok.value)
