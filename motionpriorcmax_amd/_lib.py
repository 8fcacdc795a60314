"""ctypes binding of the C ABI declared in include/mpcmax.h.

There is NO fallback: if libmpcmax.so is missing or a call fails, a RuntimeError is raised."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libmpcmax.so')
if os.environ.get('MPC_AB_LIB'):          # diagnostics: another build of the SAME library beside the product one (bounds-checked: tools/bounds_run.sh; A/B timing)
    LIB_PATH = os.path.abspath(os.environ['MPC_AB_LIB'])

# flags, mirror of include/mpcmax.h
F_SCALE_BY_DT = 1 << 0
F_MASK_BORDER = 1 << 1
F_POLARITY_SPLIT = 1 << 2
F_NORM_L2 = 1 << 3
F_OBJ_VARIANCE = 1 << 4
F_DIST_L1 = 1 << 5
F_SCHEME_IWD = 1 << 6
F_WANT_NEXT = 1 << 7
F_NO_WARP = 1 << 8
F_UNIT_WEIGHT = 1 << 9
F_ATOMIC_PATH = 1 << 10
F_NO_BWD_RECORDS = 1 << 11

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -4        # include/mpcmax.h
BASIS_POLY, BASIS_DCT, BASIS_MATRIX = 0, 1, 2
DT_F32, DT_F16, DT_BF16 = 0, 1, 2                   # include/mpcmax.h: MPC_DT_*, the element type of a `_dt` entry point's network tensor
SCAL_LOSS, SCAL_FOCUS, SCAL_SMOOTH, SCAL_VAL, SCAL_GCOEF, SCAL_COUNT = 0, 1, 2, 3, 4, 8
SCAL_PYR_RATIO = 5                                  # level_scal rows of mpc_iwe_pyramid_fwd: the fold ratio r_l

class Shape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in
                ('B', 'M', 'Mp', 'nb', 'T', 'H', 'W', 'sp', 'hq', 'wq', 'n', 'K')] + \
               [('flags', ctypes.c_uint32)]


class FocusBuffers(ctypes.Structure):
    """include/mpcmax.h: struct mpc_focus_buffers."""
    _fields_ = [(k, ctypes.c_void_p) for k in
                ('traj', 'events', 't_ref', 'flow_lut', 'flow_next', 'knn_state', 'smooth_grad', 'iwe_raw', 'iwe_blur',
                 'grad_iwe', 'scal')] + [('smooth_weight', ctypes.c_float), ('event_offsets', ctypes.c_void_p), ('scal_out', ctypes.c_void_p)]


class VoxShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'N', 'C', 'H', 'W', 'norm')] + [('quantile', ctypes.c_float), ('keep', ctypes.c_float)]


class ReprShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'N', 'C', 'H', 'W', 'int_xy', 'norm', 'Ho', 'Wo')]


class IngestShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'N', 'H', 'W', 'nb')]


WINDOW_TIME_FP32_SUFFIX, WINDOW_TIME_MINMAX64 = 0, 1        # include/mpcmax.h


class WindowShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'N', 'nb', 'time_mode', 'xy_int', 'p_int64', 'split')] + \
               [(k, ctypes.c_float) for k in ('duration_us', 'x_scale', 'y_scale')]


class FlowShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'C', 'n', 'patch', 'H', 'W')]


class ErrShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'H', 'W')]


class ValShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'M', 'd', 'h', 'w', 'H', 'W', 'C')]


CORR_MAX_LEVELS, CORR_MAX_TARGETS, CORR_MAX_RADIUS, CORR_F_LANE_PER_QUERY = 6, 16, 4, 1        # include/mpcmax.h
CORR_F_GRAD_ACCUM = 2                                   # mpc_corr_lookup_bwd: add the window cells into grad_level (include/mpcmax.h)
CBG_PLAIN, CBG_ROWS, CBG_LOOKUP = 0, 1, 2               # mpc_curve_basis_grad: the layouts of the three RAFT-spline nodes (include/mpcmax.h: MPC_CBG_*)


class CorrDesc(ctypes.Structure):
    """include/mpcmax.h: struct mpc_corr_desc (passed to the kernels by value)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'h', 'w', 'T', 'd', 'radius', 'num_levels', 'flags')] + \
               [(k, ctypes.c_int32 * CORR_MAX_LEVELS) for k in ('level_h', 'level_w', 'level_n')] + \
               [('level_target', (ctypes.c_uint8 * CORR_MAX_TARGETS) * CORR_MAX_LEVELS),
                ('level', ctypes.c_void_p * CORR_MAX_LEVELS), ('grad_level', ctypes.c_void_p * CORR_MAX_LEVELS)]


CORR_MAX_REFS = 4                                       # include/mpcmax.h: MPC_CORR_MAX_REFS


class CorrRefs(ctypes.Structure):
    """include/mpcmax.h: struct mpc_corr_refs (the references of mpc_corr_pyramid_multi_*)."""
    _fields_ = [('R', ctypes.c_int32), ('first_target', ctypes.c_int32 * (CORR_MAX_REFS + 1))] + \
               [(k, ctypes.c_void_p * CORR_MAX_REFS) for k in ('fmap1', 'fmap2', 'grad_fmap1', 'grad_fmap2')]


TARGETS_EVIMO2, TARGETS_MULTIFLOW = 0, 1        # include/mpcmax.h: mpc_targets_shape.mode


class TargetsShape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'S', 'H', 'W', 'Ho', 'Wo', 'mode', 'has_id')]


# key order of mpc_val_metrics, mirror of the MPC_VAL_* macros of include/mpcmax.h
VAL_MAX_STEPS, VAL_COUNT = 16, 75
VAL_SINGLE, VAL_MASKED_SINGLE, VAL_MULTI, VAL_EV_MASKED_MULTI, VAL_MASKED_MULTI, VAL_EPE_MULTI_LIN, VAL_AE_MULTI_LIN = 0, 5, 10, 31, 52, 73, 74
VAL_SINGLE_KEYS = ('epe', 'ae', '1pe', '2pe', '3pe')
VAL_MULTI_KEYS = ('epe_multi', 'ae_multi', 'T3PE', 'TEPE', 'TAE')          # then EPE_STEP00 .. at + 5

vp, i32, i64, f32, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_int
sp, fb, vsp, isp, wsp, cdp, tsp = (ctypes.POINTER(t) for t in (Shape, FocusBuffers, VoxShape, IngestShape, WindowShape, CorrDesc, TargetsShape))
crp = ctypes.POINTER(CorrRefs)
fsp, esp, rsp, vlp = (ctypes.POINTER(t) for t in (FlowShape, ErrShape, ReprShape, ValShape))

# The whole binding: every export of include/mpcmax.h -> (restype, argtypes), in the header's order.  lib() applies the table and
# EXPORTS is its key list, so an export cannot exist without a signature (a symbol left without argtypes would pass 64-bit
# pointers as C int: a wild GPU write, not a Python error).  tests/test_abi_and_host.py holds arity and return size against the header.
SIGNATURES = {
    'mpc_version': (cint, []),
    'mpc_last_error_string': (ctypes.c_char_p, []),
    'mpc_bounds_check': (cint, []),
    'mpc_profile_start': (cint, []),
    'mpc_profile_stop': (cint, [ctypes.c_char_p, i32, ctypes.POINTER(f32), i32]),
    'mpc_workspace_bytes': (i64, [sp]),
    'mpc_knn_lut_fwd': (cint, [sp] + [vp] * 7),
    'mpc_knn_state_floats': (i64, [sp]),
    'mpc_knn_fail_list_offset': (i64, [sp]),
    'mpc_knn_list_offsets': (cint, [sp, ctypes.POINTER(i64)]),
    'mpc_knn_tail_counters_offset': (i64, [sp]),
    'mpc_knn_lut_bwd': (cint, [sp] + [vp] * 7),
    'mpc_knn_wide_workspace_bytes': (i64, [sp]),
    'mpc_knn_merge_fwd': (cint, [sp, vp, vp, ctypes.POINTER(i32), i32] + [vp] * 4),
    'mpc_knn_idx_bwd': (cint, [sp] + [vp] * 7),
    'mpc_event_splat_fwd':(cint, [sp] + [vp] * 6),
    'mpc_event_splat_fwd_fixed': (cint, [sp] + [vp] * 6),
    'mpc_iwe_from_fixed': (cint, [vp, vp, i64, vp]),
    'mpc_contrast_fwd': (cint, [sp] + [vp] * 5),
    'mpc_lut_smooth': (cint, [sp, vp, i32, i32, f32, vp, vp, vp]),
    'mpc_finalize': (cint, [sp, i32, i32, f32, vp, vp, vp]),
    'mpc_event_pos_grad': (cint, [sp] + [vp] * 7),
    'mpc_pe_warp': (cint, [sp, vp, vp, vp, i32, vp, vp, vp]),
    'mpc_pe_grad': (cint, [sp, vp, vp, i32] + [vp] * 6),
    'mpc_pe_grad_ordered': (cint, [sp, vp, vp, vp, i32] + [vp] * 5 + [i32, vp]),
    'mpc_pe_grad_ordered_supported': (i32, [sp, i32]),
    'mpc_pe_tile_rows': (cint, [vp, vp] + [i32] * 6 + [vp]),
    'mpc_pe_tile_rows_bwd': (cint, [vp, vp] + [i32] * 6 + [vp]),
    'mpc_pe_tile_rows_dt': (cint, [vp, i32, vp] + [i32] * 6 + [vp]),
    'mpc_pe_tile_rows_bwd_dt': (cint, [vp, vp, i32] + [i32] * 6 + [vp]),
    'mpc_pe_basis_field': (cint, [vp, vp, vp] + [i32] * 4 + [vp]),
    'mpc_pe_rows_grad_finish': (cint, [vp, i32, vp, vp, vp, vp] + [i32] * 4 + [vp]),
    'mpc_pe_table_supported': (i32, [sp, i32, i32]),
    'mpc_pe_table_limit': (i32, []),
    'mpc_pe_table_warp': (cint, [sp, vp, vp, vp, i32, i32, vp, vp, vp]),
    'mpc_pe_table_grad': (cint, [sp, vp, vp, i32, i32] + [vp] * 7),
    'mpc_pe_table_grad_ordered': (cint, [sp, vp, vp, vp, i32, i32] + [vp] * 5 + [i32, vp, vp]),
    'mpc_pe_table_basis_grad': (cint, [sp, vp, vp, vp, i32, i32] + [vp] * 6),
    'mpc_pe_field_basis_grad': (cint, [vp] * 5 + [i32] * 4 + [vp]),
    'mpc_pec_supported': (i32, [sp, i32, i32, i32]),
    'mpc_pec_head_rows': (cint, [vp, vp, f32, i32, vp] + [i32] * 4 + [vp]),
    'mpc_pec_head_rows_bwd_workspace_bytes': (i64, [i32] * 5),
    'mpc_pec_head_rows_bwd': (cint, [vp, vp, vp, f32, i32, vp, vp] + [i32] * 4 + [vp, vp]),
    'mpc_pec_head_rows_dt': (cint, [vp, vp, i32, f32, i32, vp] + [i32] * 4 + [vp]),
    'mpc_pec_head_rows_bwd_dt': (cint, [vp, vp, vp, i32, f32, i32, vp, vp] + [i32] * 4 + [vp, vp]),
    'mpc_pec_warp': (cint, [sp, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
    'mpc_pec_rows_grad': (cint, [sp, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp]),
    'mpc_pec_rows_grad_passes': (i32, [sp, i32, i32]),
    'mpc_pec_field': (cint, [vp, vp, vp] + [i32] * 4 + [vp]),
    'mpc_pec_field_adjoint': (cint, [vp, vp, vp, vp] + [i32] * 4 + [vp]),
    'mpc_pec_table_basis_grad': (cint, [sp, vp, vp, vp, i32, i32] + [vp] * 6),
    'mpc_pec_field_basis_grad': (cint, [vp] * 5 + [i32] * 4 + [vp]),
    'mpc_event_splat_bwd': (cint, [sp] + [vp] * 10),
    'mpc_focus_fwd': (cint, [sp, fb, vp, vp]),
    'mpc_focus_bwd': (cint, [sp, fb] + [vp] * 6),
    'mpc_event_lut_strips': (i32, [sp]),
    'mpc_event_order_workspace_bytes': (i64, [sp]),
    'mpc_event_bucket_order': (cint, [sp] + [vp] * 5),
    'mpc_event_splat_bwd_ordered': (cint, [sp] + [vp] * 11),
    'mpc_pool2_fwd': (cint, [vp, vp, i32, i32, i32, vp]),
    'mpc_pool2_bwd_add': (cint, [vp, vp, vp, vp, i32, i32, i32, vp]),
    'mpc_iwe_pyramid_supported': (cint, [sp, i32]),
    'mpc_iwe_pyramid_workspace_bytes': (i64, [sp, i32, i32]),
    'mpc_iwe_pyramid_fwd': (cint, [sp, i32] + [vp] * 7),
    'mpc_scale': (cint, [vp, vp, vp, i64, vp]),
    'mpc_voxel_workspace_bytes': (i64, [vsp]),
    'mpc_voxel_grid': (cint, [vsp] + [vp] * 5),
    'mpc_repr_workspace_bytes': (i64, [rsp]),
    'mpc_repr_grid': (cint, [rsp] + [vp] * 9),
    'mpc_repr_norm_workspace_bytes': (i64, [i32]),
    'mpc_repr_norm': (cint, [vp, i32, i64, vp, vp]),
    'mpc_ingest_workspace_bytes': (i64, [isp]),
    'mpc_ingest_count': (cint, [isp] + [vp] * 8),
    'mpc_ingest_scatter': (cint, [isp] + [vp] * 5 + [i32, i32] + [vp] * 4),
    'mpc_ingest_ordered_workspace_bytes': (i64, [isp, sp]),
    'mpc_ingest_scatter_ordered': (cint, [isp, sp] + [vp] * 5 + [i32, i32] + [vp] * 6),
    'mpc_ingest_rect_count': (cint, [isp, i32, i32] + [vp] * 9),
    'mpc_ingest_rect_scatter': (cint, [isp, i32, i32] + [vp] * 6 + [i32, i32] + [vp] * 4),
    'mpc_ingest_rect_scatter_ordered': (cint, [isp, sp, i32, i32] + [vp] * 6 + [i32, i32] + [vp] * 6),
    'mpc_ingest_window_workspace_bytes': (i64, [wsp]),
    'mpc_ingest_window_count': (cint, [wsp] + [vp] * 6),
    'mpc_ingest_window_scatter': (cint, [wsp] + [vp] * 6 + [i32, i32] + [vp] * 3),
    'mpc_dense_flow': (cint, [fsp] + [vp] * 5),
    'mpc_flow_error_workspace_bytes': (i64, [esp]),
    'mpc_flow_error': (cint, [esp] + [vp] * 7),
    'mpc_curve_traj_fwd': (cint, [vp, vp, vp, f32, vp] + [i32] * 4 + [vp]),
    'mpc_curve_traj_bwd': (cint, [vp, vp, f32, vp] + [i32] * 4 + [vp]),
    'mpc_cvx_traj_fwd': (cint, [vp, vp, vp, f32, vp] + [i32] * 6 + [vp]),
    'mpc_cvx_traj_bwd_workspace_bytes': (i64, [i32] * 6),
    'mpc_cvx_traj_bwd': (cint, [vp, vp, vp, vp, f32, vp, vp] + [i32] * 6 + [vp, vp]),
    'mpc_cvx_flow_fwd': (cint, [vp, vp, vp, f32, vp] + [i32] * 5 + [vp]),
    'mpc_cvx_traj_fwd_dt': (cint, [vp, vp, i32, vp, f32, vp] + [i32] * 6 + [vp]),
    'mpc_cvx_flow_fwd_dt': (cint, [vp, vp, i32, vp, f32, vp] + [i32] * 5 + [vp]),
    'mpc_cvx_traj_bwd_dt': (cint, [vp, vp, vp, i32, vp, f32, vp, vp] + [i32] * 6 + [vp, vp]),
    'mpc_grid_traj_scratch_floats': (i64, [i32] * 6),
    'mpc_grid_traj_fwd': (cint, [vp, vp, vp, i32, f32, i32, vp, vp] + [i32] * 7 + [vp]),
    'mpc_grid_traj_bwd': (cint, [vp, vp, vp, i32, f32, vp, vp, vp, vp] + [i32] * 7 + [vp]),
    'mpc_grid_traj_fwd_dt': (cint, [vp, i32, vp, vp, i32, f32, i32, vp, vp] + [i32] * 7 + [vp]),
    'mpc_grid_traj_bwd_dt': (cint, [vp, vp, vp, i32, f32, vp, vp, i32, vp, vp] + [i32] * 7 + [vp]),
    'mpc_val_metrics_workspace_bytes': (i64, [vlp]),
    'mpc_val_metrics': (cint, [vlp, vp, vp, vp, vp, f32] + [vp] * 9),
    'mpc_corr_lookup_supported': (cint, [cdp]),
    'mpc_corr_lookup_fwd': (cint, [cdp] + [vp] * 5),
    'mpc_corr_lookup_bwd': (cint, [cdp] + [vp] * 7),
    'mpc_curve_basis_grad_scratch_floats': (i64, [i32] * 4),
    'mpc_curve_basis_grad': (cint, [vp, vp, i32, f32, vp, vp] + [i32] * 4 + [vp]),
    'mpc_corr_pyramid_workspace_bytes': (ctypes.c_longlong, [cdp, cint, cint]),
    'mpc_corr_pyramid_supported': (cint, [cdp, cint]),
    'mpc_corr_pyramid_fwd': (cint, [cdp, cint] + [vp] * 4),
    'mpc_corr_pyramid_bwd': (cint, [cdp, cint] + [vp] * 6),
    'mpc_corr_pyramid_multi_workspace_bytes': (ctypes.c_longlong, [cdp, cint, crp, cint]),
    'mpc_corr_pyramid_multi_supported': (cint, [cdp, cint, crp]),
    'mpc_corr_pyramid_multi_fwd': (cint, [cdp, cint, crp, vp, vp]),
    'mpc_corr_pyramid_multi_bwd': (cint, [cdp, cint, crp, vp, vp]),
    'mpc_corr_pyramid_fwd_dt': (cint, [cdp, cint, vp, vp, i32, vp, vp]),
    'mpc_corr_pyramid_bwd_dt': (cint, [cdp, cint] + [vp] * 4 + [i32, vp, vp]),
    'mpc_corr_pyramid_multi_fwd_dt': (cint, [cdp, cint, crp, i32, vp, vp]),
    'mpc_corr_pyramid_multi_bwd_dt': (cint, [cdp, cint, crp, i32, vp, vp]),
    'mpc_flow_targets_supported': (cint, [tsp]),
    'mpc_flow_targets': (cint, [tsp] + [vp] * 6),
    'mpc_dsec_flow_decode': (cint, [vp, vp, vp, i32, i32, i32, vp]),
    'mpc_dsec_flow_error_workspace_bytes': (i64, [esp]),
    'mpc_dsec_flow_error': (cint, [esp] + [vp] * 6),
    'mpc_dsec_flow_encode': (cint, [vp, f32, vp, i32, i32, i32, vp]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -m motionpriorcmax_amd.build` '
            '(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for this path.')
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.mpc_version() != 107:
        raise RuntimeError(f'libmpcmax.so version {L.mpc_version()} does not match the binding (107)')
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().mpc_last_error_string().decode(errors='replace')
        raise RuntimeError(f'{what} failed (rc={rc}): {msg}')
