"""ctypes binding of libbsmrocm.so -- the C ABI declared in include/bsm_rocm.h.

There is NO CPU fallback: if the HIP library is missing or a call fails, an exception is
raised.  (The CPU oracle under oracle/ is test infrastructure and is never imported here.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSM_LIB", os.path.join(_HERE, "libbsmrocm.so"))  # BSM_LIB: developer A/B builds

BSM_F32, BSM_F64, BSM_C64, BSM_C128 = 0, 1, 2, 3
# mixed precision: double / complex double vectors over values stored as float / complex float (include/bsm_rocm.h)
BSM_F64_F32, BSM_C128_C64 = 4, 5
BSM_OP_N, BSM_OP_T, BSM_OP_C = 0, 1, 2
BSM_MEM_HOST, BSM_MEM_DEVICE = 0, 1
BSM_SCHED_SERIAL, BSM_SCHED_DYNAMIC = 0, 1
BSM_ACC_AUTO, BSM_ACC_ATOMIC, BSM_ACC_COLORED, BSM_ACC_GATHER, BSM_ACC_DIRECT = 0, 1, 2, 3, 4
BSM_DEVICE_CURRENT, BSM_DEVICE_NONE = -1, -2
BSM_COLOR_WORKSTREAM_DSATUR, BSM_COLOR_DSATUR = 0, 1
# bsm_invert_blocks: largest n * n * sizeof(T) eliminated in LDS, largest order it takes (include/bsm_rocm.h)
BSM_INVERT_LDS_BYTES, BSM_INVERT_MAX_N = 131072, 1024
# bsm_eigh_blocks: largest 2 * n * n * sizeof(T) kept in LDS, largest order, the sweep cap; bsm_spectral_blocks' func
BSM_EIGH_LDS_BYTES, BSM_EIGH_MAX_N, BSM_EIGH_MAX_SWEEPS = 131072, 512, 60
BSM_SPEC_VALUES, BSM_SPEC_INV, BSM_SPEC_ABSINV, BSM_SPEC_PINV = 0, 1, 2, 3
BSM_GMRES_MAX_RESTART = 128  # bsm_gmres_create's restart, bsm_krylov_orth's k (include/bsm_rocm.h)
BSM_CG_MAX_RHS = 16  # bsm_cg_create's nrhs_max (include/bsm_rocm.h)
BSM_CG_METHOD_CG, BSM_CG_METHOD_COCG = 0, 1
BSM_POLY_MAX_STEPS = 64  # bsm_poly_create's steps (include/bsm_rocm.h)
BSM_EIGSH_LA, BSM_EIGSH_SA, BSM_EIGSH_BE, BSM_EIGSH_LM = 0, 1, 2, 3  # bsm_eigsh_params.which (include/bsm_rocm.h)
BSM_SVDS_LM, BSM_SVDS_SM = 0, 1  # bsm_svds_params.which (include/bsm_rocm.h)
(BSM_BK_VBCRS_PERM, BSM_BK_VBCRS_ROWPTR, BSM_BK_VBCRS_COLINDICES, BSM_BK_VBCRS_ROWINDICES,
 BSM_BK_COLORS, BSM_BK_TRANSPOSECOLORS, BSM_BK_DIAGONALCOLORS) = range(7)


class BsmOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("scheduler", C.c_int32),
                ("accumulate", C.c_int32), ("validate", C.c_int32), ("transpose_image", C.c_int32),
                ("own_lo", C.c_int64), ("own_hi", C.c_int64), ("ctx", C.c_void_p),
                ("blocks_memspace", C.c_int64), ("coloring", C.c_int64), ("reserved", C.c_int64 * 1)]


class BsmPartInfo(C.Structure):
    _fields_ = [("device", C.c_int32), ("reserved32", C.c_int32), ("own_lo", C.c_int64), ("own_hi", C.c_int64),
                ("touched_lo", C.c_int64), ("touched_hi", C.c_int64), ("device_bytes", C.c_int64),
                ("nblocks", C.c_int64), ("col_lo", C.c_int64), ("col_hi", C.c_int64), ("reserved", C.c_int64 * 2)]


class BsmStats(C.Structure):
    _fields_ = [("nnz", C.c_int64), ("stored_entries", C.c_int64), ("alg_bytes", C.c_int64),
                ("device_bytes", C.c_int64), ("npanels", C.c_int64), ("ntasks", C.c_int64),
                ("nworkgroups", C.c_int64), ("exclusive", C.c_int64), ("win_emissions", C.c_int64),
                ("win_inside", C.c_int64), ("win_flushed", C.c_int64), ("reserved", C.c_int64 * 5)]


class BsmGmresParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("use_x0", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("maxiter", C.c_int64), ("history_capacity", C.c_int64)]


class BsmGmresInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("cycles", C.c_int32), ("iterations", C.c_int64), ("residual", C.c_double),
                ("bnorm", C.c_double), ("a_products", C.c_int64), ("m_products", C.c_int64),
                ("workspace_bytes", C.c_int64), ("workspace", C.c_uint64)]


class BsmCgParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("use_x0", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("maxiter", C.c_int64), ("history_capacity", C.c_int64)]


class BsmLsqrParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("use_x0", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double), ("ntol", C.c_double),
                ("damp", C.c_double), ("maxiter", C.c_int64), ("history_capacity", C.c_int64)]


class BsmCgInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("columns_converged", C.c_int32), ("iterations", C.c_int64),
                ("a_products", C.c_int64), ("m_products", C.c_int64), ("workspace_bytes", C.c_int64),
                ("workspace", C.c_uint64)]


class BsmCgColumn(C.Structure):
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("iterations", C.c_int64), ("residual", C.c_double),
                ("bnorm", C.c_double)]


class BsmEigshParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("maxcycles", C.c_int32), ("vectors", C.c_int32)]


class BsmEigshInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("nconv", C.c_int32), ("cycles", C.c_int32), ("reserved", C.c_int32),
                ("a_products", C.c_int64), ("anorm", C.c_double), ("workspace_bytes", C.c_int64), ("workspace", C.c_uint64)]


class BsmEigshPair(C.Structure):
    _fields_ = [("value", C.c_double), ("estimate", C.c_double), ("residual", C.c_double)]


class BsmSvdsParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("maxcycles", C.c_int32), ("vectors", C.c_int32)]


class BsmSvdsInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("nconv", C.c_int32), ("cycles", C.c_int32), ("reserved", C.c_int32),
                ("a_products", C.c_int64), ("anorm", C.c_double), ("workspace_bytes", C.c_int64), ("workspace", C.c_uint64)]


class BsmSvdsTriplet(C.Structure):
    _fields_ = [("value", C.c_double), ("estimate", C.c_double), ("residual_av", C.c_double), ("residual_ahu", C.c_double)]


class BsmLobpcgParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("maxiter", C.c_int32), ("reserved", C.c_int32)]


class BsmLobpcgInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("nconv", C.c_int32), ("iterations", C.c_int32), ("drops", C.c_int32),
                ("a_products", C.c_int64), ("m_products", C.c_int64), ("anorm", C.c_double), ("workspace_bytes", C.c_int64)]


class BsmError(RuntimeError):
    pass


_PP = C.POINTER(C.c_void_p)
_I64P = C.POINTER(C.c_int64)
_lib = None

# every symbol include/bsm_rocm.h declares
EXPORTS = ["bsm_options_default", "bsm_vbcrs_create", "bsm_vbcrs_create_from_symmetric",
           "bsm_vbcrs_create_from_blocksparse", "bsm_ctx_create", "bsm_ctx_destroy", "bsm_ctx_devices",
           "bsm_partition_rows", "bsm_part_info", "bsm_host_register", "bsm_host_unregister", "bsm_rowcolvals",
           "bsm_blocksparse_create",
           "bsm_symmetric_create", "bsm_mul", "bsm_mul_multi", "bsm_mul_parts",
           "bsm_mul_cvec", "bsm_mul_multi_cvec", "bsm_get_bookkeeping", "bsm_get_image", "bsm_stats",
           "bsm_color", "bsm_destroy", "bsm_last_error", "bsm_version",
           "bsm_vec_add_segments", "bsm_stream_create_reserved", "bsm_stream_destroy", "bsm_update_blocks", "bsm_value_passes",
           "bsm_submatrices", "bsm_diag", "bsm_invert_blocks", "bsm_eigh_blocks", "bsm_spectral_blocks",
           "bsm_krylov_orth_work", "bsm_krylov_orth", "bsm_gmres_create", "bsm_gmres_solve",
           "bsm_gmres_destroy", "bsm_cg_create", "bsm_cg_solve", "bsm_cg_destroy", "bsm_bicgstab_create", "bsm_bicgstab_solve",
           "bsm_bicgstab_destroy", "bsm_gmres_multi_create", "bsm_gmres_multi_solve", "bsm_gmres_multi_destroy",
           "bsm_minres_create", "bsm_minres_solve", "bsm_minres_destroy", "bsm_lsqr_create", "bsm_lsqr_solve", "bsm_lsqr_destroy",
           "bsm_poly_create", "bsm_poly_info", "bsm_krylov_combine_tile", "bsm_krylov_combine", "bsm_eigsh_create",
           "bsm_eigsh_solve", "bsm_eigsh_destroy", "bsm_block_gram_grid", "bsm_block_gram_work", "bsm_block_gram",
           "bsm_block_combine_tile", "bsm_block_combine", "bsm_lobpcg_create", "bsm_lobpcg_solve", "bsm_lobpcg_destroy",
           "bsm_svds_create", "bsm_svds_solve", "bsm_svds_destroy"]


# include/bsm_synth.h (bench / test utility: synthetic operators generated in HBM)
SYNTH_EXPORTS = ["bsm_synth_blocks", "bsm_synth_vector", "bsm_bench_stream"]


def lib():
    """Loads libbsmrocm.so once; raises loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        # compile on demand (hipcc --offload-arch=gfx950, in-tree); this is a build step, not a
        # fallback: without the HIP library nothing below works
        import fcntl
        import subprocess
        try:
            # one builder at a time: the ranks of a multi-GPU job may all arrive here together
            with open(os.path.join(_HERE, "csrc", ".build.lock"), "w") as lk:
                fcntl.flock(lk, fcntl.LOCK_EX)
                if not os.path.exists(LIB_PATH):
                    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the product path.")
    L = C.CDLL(LIB_PATH)
    L.bsm_options_default.argtypes = [C.POINTER(BsmOptions)]
    L.bsm_options_default.restype = None
    L.bsm_vbcrs_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, _PP, _I64P, _I64P,
                                   _I64P, _I64P, _I64P, C.POINTER(BsmOptions),
                                   C.POINTER(C.c_void_p)]
    L.bsm_blocksparse_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, _PP, _I64P,
                                         _I64P, _I64P, _PP, _PP, C.POINTER(BsmOptions),
                                         C.POINTER(C.c_void_p)]
    L.bsm_symmetric_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, _PP, _I64P,
                                       _I64P, _PP, C.c_int64, _PP, _I64P, _I64P, _I64P, _PP,
                                       _PP, C.POINTER(BsmOptions), C.POINTER(C.c_void_p)]
    L.bsm_vbcrs_create_from_symmetric.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, _PP, _I64P,
                                                  _I64P, _I64P, C.c_int64, _PP, _I64P, _I64P, _I64P,
                                                  _I64P, _I64P, C.POINTER(BsmOptions),
                                                  C.POINTER(C.c_void_p)]
    L.bsm_vbcrs_create_from_blocksparse.argtypes = L.bsm_blocksparse_create.argtypes
    _I32P = C.POINTER(C.c_int32)
    L.bsm_ctx_create.argtypes = [_I32P, C.c_int32, C.POINTER(C.c_void_p)]
    L.bsm_ctx_destroy.argtypes = [C.c_void_p]
    L.bsm_ctx_devices.argtypes = [C.c_void_p, _I32P, _I32P, C.c_int32]
    L.bsm_partition_rows.argtypes = [C.c_int64, C.c_int64, _I64P, _I64P, C.c_int32, _I32P, _I64P, _I64P]
    L.bsm_part_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(BsmPartInfo)]
    for name in ("bsm_vbcrs_create_from_blocksparse", "bsm_ctx_create", "bsm_ctx_destroy", "bsm_ctx_devices",
                 "bsm_partition_rows", "bsm_part_info"):
        getattr(L, name).restype = C.c_int
    L.bsm_rowcolvals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _I64P, C.c_int, C.c_void_p]
    L.bsm_rowcolvals.restype = C.c_int
    L.bsm_stream_create_reserved.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.bsm_stream_destroy.argtypes = [C.c_void_p]
    L.bsm_stream_create_reserved.restype = L.bsm_stream_destroy.restype = C.c_int
    L.bsm_vec_add_segments.argtypes = [C.c_int, C.c_void_p, C.c_int32, _I64P, _PP, _I64P, C.c_void_p]
    L.bsm_vec_add_segments.restype = C.c_int
    L.bsm_host_register.argtypes = [C.c_void_p, C.c_int64]
    L.bsm_host_unregister.argtypes = [C.c_void_p]
    L.bsm_host_register.restype = L.bsm_host_unregister.restype = C.c_int
    L.bsm_synth_blocks.argtypes = [C.c_int, C.c_uint64, C.c_int64, _I64P, _I64P, _I64P, _I32P, _PP, C.c_void_p]
    L.bsm_synth_vector.argtypes = [C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.bsm_synth_blocks.restype = L.bsm_synth_vector.restype = C.c_int
    if hasattr(L, "bsm_bench_stream") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate it)
        L.bsm_bench_stream.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.bsm_bench_stream.restype = C.c_int
    L.bsm_mul.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_int, C.c_int, C.c_void_p]
    L.bsm_mul_multi.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.bsm_mul_multi.restype = C.c_int
    if hasattr(L, "bsm_mul_cvec") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        L.bsm_mul_cvec.argtypes = L.bsm_mul.argtypes
        L.bsm_mul_multi_cvec.argtypes = L.bsm_mul_multi.argtypes
        L.bsm_mul_cvec.restype = L.bsm_mul_multi_cvec.restype = C.c_int
    if hasattr(L, "bsm_mul_parts") or "BSM_LIB" not in os.environ:
        L.bsm_mul_parts.argtypes = [C.c_void_p, C.c_int, _PP, _PP, C.c_void_p, C.c_void_p, C.c_int, _PP]
        L.bsm_mul_parts.restype = C.c_int
    if hasattr(L, "bsm_update_blocks") or "BSM_LIB" not in os.environ:
        L.bsm_update_blocks.argtypes = [C.c_void_p, C.c_int64, _I64P, _PP, _I64P, C.c_int, C.c_void_p]
        L.bsm_update_blocks.restype = C.c_int
    L.bsm_get_bookkeeping.argtypes = [C.c_void_p, C.c_int, _I64P, _I64P]
    L.bsm_get_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _I64P]
    L.bsm_color.argtypes = [C.c_int64, _PP, _I64P, C.c_int, _I64P, _I64P]
    L.bsm_color.restype = C.c_int
    L.bsm_stats.argtypes = [C.c_void_p, C.POINTER(BsmStats)]
    if hasattr(L, "bsm_value_passes") or "BSM_LIB" not in os.environ:
        L.bsm_value_passes.argtypes = [C.c_void_p, _I64P]
        L.bsm_value_passes.restype = C.c_int
    if hasattr(L, "bsm_submatrices") or "BSM_LIB" not in os.environ:
        L.bsm_submatrices.argtypes = [C.c_void_p, C.c_int, C.c_int64, _PP, _I64P, _PP, _I64P, _PP, _I64P, C.c_int, C.c_void_p]
        L.bsm_diag.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bsm_submatrices.restype = L.bsm_diag.restype = C.c_int
    if hasattr(L, "bsm_invert_blocks") or "BSM_LIB" not in os.environ:
        L.bsm_invert_blocks.argtypes = [C.c_int, C.c_int64, _PP, _I64P, _I64P, _I64P, C.c_int, C.c_void_p]
        L.bsm_invert_blocks.restype = C.c_int
    if hasattr(L, "bsm_eigh_blocks") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        L.bsm_eigh_blocks.argtypes = [C.c_int, C.c_int64, _PP, _I64P, _I64P, _PP, C.c_int32, _I64P, _I32P, C.c_int, C.c_void_p]
        # bsm_spectral_blocks takes a double BY VALUE: it keeps argtypes = None (the static mirror check of the suite classes
        # integers and pointers only) and is called through spectral_blocks_call below, which converts every argument itself
        L.bsm_eigh_blocks.restype = L.bsm_spectral_blocks.restype = C.c_int
    if hasattr(L, "bsm_gmres_create") or "BSM_LIB" not in os.environ:
        L.bsm_krylov_orth_work.argtypes = [C.c_int, C.c_int64, C.c_int64]
        L.bsm_krylov_orth_work.restype = C.c_int64
        L.bsm_krylov_orth.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.bsm_gmres_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_gmres_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BsmGmresParams),
                                      C.POINTER(BsmGmresInfo), C.POINTER(C.c_double), C.c_int, C.c_void_p]
        L.bsm_gmres_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_krylov_orth", "bsm_gmres_create", "bsm_gmres_solve", "bsm_gmres_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_cg_create") or "BSM_LIB" not in os.environ:
        L.bsm_cg_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_cg_solve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(BsmCgParams),
                                   C.POINTER(BsmCgInfo), C.POINTER(BsmCgColumn), C.POINTER(C.c_double), C.c_int, C.c_void_p]
        L.bsm_cg_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_cg_create", "bsm_cg_solve", "bsm_cg_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_bicgstab_create") or "BSM_LIB" not in os.environ:  # (the structs are those of bsm_cg_*)
        L.bsm_bicgstab_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_bicgstab_solve.argtypes = L.bsm_cg_solve.argtypes
        L.bsm_bicgstab_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_bicgstab_create", "bsm_bicgstab_solve", "bsm_bicgstab_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_gmres_multi_create") or "BSM_LIB" not in os.environ:  # (the structs are those of bsm_cg_*)
        L.bsm_gmres_multi_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32,
                                             C.POINTER(C.c_void_p)]
        L.bsm_gmres_multi_solve.argtypes = L.bsm_cg_solve.argtypes
        L.bsm_gmres_multi_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_gmres_multi_create", "bsm_gmres_multi_solve", "bsm_gmres_multi_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_minres_create") or "BSM_LIB" not in os.environ:  # (the structs are those of bsm_cg_*)
        L.bsm_minres_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_minres_solve.argtypes = L.bsm_cg_solve.argtypes
        L.bsm_minres_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_minres_create", "bsm_minres_solve", "bsm_minres_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_lsqr_create") or "BSM_LIB" not in os.environ:  # (info and columns are those of bsm_cg_*)
        L.bsm_lsqr_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_lsqr_solve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(BsmLsqrParams),
                                     C.POINTER(BsmCgInfo), C.POINTER(BsmCgColumn), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_int, C.c_void_p]
        L.bsm_lsqr_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_lsqr_create", "bsm_lsqr_solve", "bsm_lsqr_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_poly_create") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        _F64P = C.POINTER(C.c_double)
        L.bsm_poly_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, _F64P, _F64P,
                                      C.POINTER(C.c_void_p)]
        L.bsm_poly_info.argtypes = [C.c_void_p, _I32P, _F64P, _F64P, _I64P]
        L.bsm_poly_create.restype = L.bsm_poly_info.restype = C.c_int
    if hasattr(L, "bsm_eigsh_create") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        L.bsm_krylov_combine_tile.argtypes = [C.c_int, C.c_int64]
        L.bsm_krylov_combine_tile.restype = C.c_int64
        L.bsm_krylov_combine.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.bsm_eigsh_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_eigsh_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BsmEigshParams), C.POINTER(BsmEigshInfo),
                                      C.POINTER(BsmEigshPair), C.c_int, C.c_void_p]
        L.bsm_eigsh_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_krylov_combine", "bsm_eigsh_create", "bsm_eigsh_solve", "bsm_eigsh_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_lobpcg_create") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        L.bsm_block_gram_grid.argtypes = [C.c_int, C.c_int64]
        L.bsm_block_gram_work.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64]
        L.bsm_block_combine_tile.argtypes = [C.c_int, C.c_int64]
        L.bsm_block_gram_grid.restype = L.bsm_block_gram_work.restype = L.bsm_block_combine_tile.restype = C.c_int64
        L.bsm_block_gram.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p]
        L.bsm_block_combine.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p]
        L.bsm_lobpcg_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_lobpcg_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(BsmLobpcgParams),
                                       C.POINTER(BsmLobpcgInfo), C.POINTER(BsmEigshPair), C.POINTER(C.c_double), C.c_int64, C.c_int,
                                       C.c_void_p]
        L.bsm_lobpcg_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_block_gram", "bsm_block_combine", "bsm_lobpcg_create", "bsm_lobpcg_solve", "bsm_lobpcg_destroy"):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "bsm_svds_create") or "BSM_LIB" not in os.environ:  # (developer A/B builds may predate them)
        L.bsm_svds_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.bsm_svds_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(BsmSvdsParams),
                                     C.POINTER(BsmSvdsInfo), C.POINTER(BsmSvdsTriplet), C.c_int, C.c_void_p]
        L.bsm_svds_destroy.argtypes = [C.c_void_p]
        for name in ("bsm_svds_create", "bsm_svds_solve", "bsm_svds_destroy"):
            getattr(L, name).restype = C.c_int
    L.bsm_destroy.argtypes = [C.c_void_p]
    L.bsm_last_error.restype = C.c_char_p
    L.bsm_version.restype = C.c_char_p
    for name in ("bsm_vbcrs_create", "bsm_vbcrs_create_from_symmetric", "bsm_blocksparse_create", "bsm_symmetric_create", "bsm_mul",
                 "bsm_get_bookkeeping", "bsm_get_image", "bsm_stats", "bsm_destroy"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


def spectral_blocks_call(dtype, nblocks, V, n, ldv, w, func, rcond, out, ldo, info, memspace, stream):
    """bsm_spectral_blocks with every argument converted here (lib(): why it has no argtypes).  V, w, out: void* arrays; n,
    ldv, ldo, info: int64 pointers (info may be None)"""
    return lib().bsm_spectral_blocks(C.c_int(dtype), C.c_int64(nblocks), V, n, ldv, w, C.c_int32(func), C.c_double(rcond), out, ldo,
                                     info, C.c_int(memspace), C.c_void_p(stream))


def check(rc):
    if rc != 0:
        raise BsmError(f"libbsmrocm error {rc}: {lib().bsm_last_error().decode()}")
