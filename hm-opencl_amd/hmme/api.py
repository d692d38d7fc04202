"""ctypes bindings onto the C ABI (include/hmme.h) of libhmme.so -- the HIP engine.

There is no CPU fallback: `load()` raises if the library is missing, and every call that needs
the GPU raises HmmeError carrying the engine's own error text.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
LIB_PATH = os.environ.get("HMME_LIB", os.path.join(CSRC, "libhmme.so"))   # HMME_LIB: A/B builds of the kernel
NUM_PARTS = 593

# every symbol include/hmme.h declares (tests check the library exports all of them)
SYMBOLS = ["hmme_create", "hmme_destroy", "hmme_last_error", "hmme_device_info", "hmme_set_lambda",
           "hmme_set_lambda_q16", "hmme_get_lambda_q16", "hmme_params_ocl_compat", "hmme_set_search_range",
           "hmme_slot_index", "hmme_slot_rect", "hmme_slot_index_amp_off", "hmme_amp_off_slot", "hmme_compact_amp_off", "hmme_search_ctu", "hmme_search_ctu_w", "hmme_search_refine_ctu_w", "hmme_refine_ctu_w", "hmme_search_refine_ctu", "hmme_refine_ctu", "hmme_plane_create", "hmme_plane_create_ex", "hmme_plane_bit_depth", "hmme_plane_destroy", "hmme_plane_upload_pel",
           "hmme_plane_upload_u8", "hmme_host_register", "hmme_host_unregister", "hmme_plane_set_device_u8", "hmme_plane_width", "hmme_plane_height",
           "hmme_num_ctus", "hmme_search_frame", "hmme_search_frame_device", "hmme_search_frame_multi",
           "hmme_search_frame_multi_device", "hmme_refine_frame", "hmme_refine_frame_multi_device",
           "hmme_search_pairs_device", "hmme_refine_pairs_device", "hmme_plane_upload_async",
           "hmme_upload_status", "hmme_abi_version", "hmme_build_id", "hmme_device_index", "hmme_set_error_printing",
           "hmme_weight_check", "hmme_search_pairs_w_device", "hmme_refine_pairs_w_device", "hmme_search_frame_w", "hmme_refine_frame_w",
           "hmme_bipred_check", "hmme_predict_pairs_device", "hmme_predict_frame", "hmme_search_pairs_bi_device", "hmme_refine_pairs_bi_device",
           "hmme_search_frame_bi", "hmme_refine_frame_bi",
           "hmme_bipred_weight_check", "hmme_predict_pairs_w_device", "hmme_predict_frame_w", "hmme_search_pairs_bi_w_device",
           "hmme_refine_pairs_bi_w_device", "hmme_search_frame_bi_w", "hmme_refine_frame_bi_w",
           "hmme_slot_key", "hmme_select_check", "hmme_select_pairs_device", "hmme_select_frame",
           "hmme_ref_idx_bits", "hmme_select_refs_check", "hmme_select_refs_device", "hmme_select_refs_frame",
           "hmme_predict_refs_device", "hmme_predict_refs_frame",
           "hmme_select_dirs_check", "hmme_select_dirs_device", "hmme_select_dirs_frame", "hmme_predict_bi_device", "hmme_predict_bi_frame",
           "hmme_predict_bi_weight_check", "hmme_predict_bi_w_device", "hmme_predict_bi_w_frame", "hmme_predict_refs_w_device", "hmme_predict_refs_w_frame",
           "hmme_plane_stats", "hmme_wp_estimate", "hmme_wp_estimate_420",
           "hmme_predict_chroma_pairs_device", "hmme_predict_chroma_frame", "hmme_predict_chroma_refs_device", "hmme_predict_chroma_refs_frame",
           "hmme_predict_refs4_device", "hmme_predict_refs4_frame", "hmme_predict_chroma_refs4_device", "hmme_predict_chroma_refs4_frame",
           "hmme_predict_chroma_bi_device", "hmme_predict_chroma_bi_frame",
           "hmme_residual_pairs_device", "hmme_residual_frame",
           "hmme_search_frame_bi_refs_device", "hmme_refine_frame_bi_refs_device", "hmme_search_frame_bi_refs", "hmme_refine_frame_bi_refs",
           "hmme_select_dirs_refs_check", "hmme_select_dirs_refs_device", "hmme_select_dirs_refs_frame",
           "hmme_predict_bi_refs_device", "hmme_predict_bi_refs_frame",
           "hmme_bipred_refs_weight_check", "hmme_search_frame_bi_refs_w_device", "hmme_refine_frame_bi_refs_w_device", "hmme_search_frame_bi_refs_w",
           "hmme_refine_frame_bi_refs_w",
           "hmme_predict_bi_refs_weight_check", "hmme_predict_bi_refs_w_device", "hmme_predict_bi_refs_w_frame",
           "hmme_predict_chroma_bi_refs_device", "hmme_predict_chroma_bi_refs_frame",
           "hmme_search_pairs_bi4_device", "hmme_refine_pairs_bi4_device", "hmme_search_frame_bi4", "hmme_refine_frame_bi4",
           "hmme_select_dirs4_check", "hmme_select_dirs4_device", "hmme_select_dirs4_frame",
           "hmme_predict_bi4_device", "hmme_predict_bi4_frame", "hmme_predict_chroma_bi4_device", "hmme_predict_chroma_bi4_frame",
           "hmme_search_frame_bi_refs4_device", "hmme_refine_frame_bi_refs4_device", "hmme_search_frame_bi_refs4", "hmme_refine_frame_bi_refs4",
           "hmme_select_dirs_refs4_check", "hmme_select_dirs_refs4_device", "hmme_select_dirs_refs4_frame",
           "hmme_predict_bi_refs4_device", "hmme_predict_bi_refs4_frame", "hmme_predict_chroma_bi_refs4_device", "hmme_predict_chroma_bi_refs4_frame"]
# test / measurement entry points (include/hmme_test.h): not part of the boundary
TEST_SYMBOLS = ["hmme_test_time_search_kernel", "hmme_test_device_address", "hmme_test_frac_deal", "hmme_test_tail_plan", "hmme_test_stage_layout", "hmme_test_picture_job", "hmme_test_time_weight_passes", "hmme_test_time_bipred_origin",
                "hmme_test_time_wp_estimate_passes", "hmme_test_pk_gate", "hmme_test_pk_body", "hmme_test_pk_task_marker_free", "hmme_test_pk_task_full",
                "hmme_test_task_carry_fits", "hmme_test_carry_index", "hmme_test_carry_position",
                "hmme_test_wp_parameters", "hmme_test_wp_select", "hmme_test_ctu_plan"]
ABI_VERSION = 6   # HMME_ABI_VERSION of the include/hmme.h these bindings were written against


class HmmeError(RuntimeError):
    pass


class SearchParams(C.Structure):
    _fields_ = [("lt_x", C.c_int), ("lt_y", C.c_int), ("rb_x", C.c_int), ("rb_y", C.c_int),
                ("pred_x", C.c_int), ("pred_y", C.c_int), ("fen", C.c_int), ("bit_depth", C.c_int),
                ("shift_free", C.c_int)]


class Weight(C.Structure):
    """hmme_weight: luma WPScalingParam of the reference picture"""
    _fields_ = [("w0", C.c_int), ("offset", C.c_int), ("shift", C.c_int), ("round", C.c_int)]


class WpInfo(C.Structure):
    """hmme_wp_info: how hmme_wp_estimate arrived at one reference's weight (WeightPredAnalysis.cpp; the rule: include/hmme.h)"""
    _fields_ = [("cur_dc_sum", C.c_int64), ("cur_ac", C.c_int64), ("ref_dc_sum", C.c_int64), ("ref_ac", C.c_int64),
                ("sad_wp", C.c_int64), ("sad_nowp", C.c_int64),
                ("log2_denom", C.c_int), ("weight", C.c_int), ("offset", C.c_int), ("present", C.c_int),
                ("served_search", C.c_int), ("served_refine", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SelectParams(C.Structure):
    """hmme_select_params: the partition decision over the 593-slot tables (the rule: include/hmme.h)"""
    _fields_ = [("mv_per_ctu", C.c_int), ("mv_unit", C.c_int), ("price_mv", C.c_int), ("part_mask", C.c_uint),
                ("min_depth", C.c_int), ("max_depth", C.c_int), ("cu_cost", C.c_uint32), ("pu_cost", C.c_uint32)]

    def __init__(self, mv_per_ctu=64, mv_unit=0, price_mv=0, part_mask=0xF7, min_depth=0, max_depth=3, cu_cost=0, pu_cost=0):
        super().__init__(int(mv_per_ctu), int(mv_unit), int(price_mv), int(part_mask), int(min_depth), int(max_depth), int(cu_cost), int(pu_cost))


class DirParams(C.Structure):
    """hmme_dir_params: the caller's bit counts of the L0 / L1 / bi decision (the rule: include/hmme.h): dir_bits = HM's uiMbBits[3],
    list_bits = reference-index + MVP-index bits of list 0 and list 1"""
    _fields_ = [("dir_bits", C.c_uint32 * 3), ("list_bits", C.c_uint32 * 2)]

    def __init__(self, dir_bits=(0, 0, 0), list_bits=(0, 0)):
        super().__init__((C.c_uint32 * 3)(*[int(v) for v in dir_bits]), (C.c_uint32 * 2)(*[int(v) for v in list_bits]))


class DirRefsParams(C.Structure):
    """hmme_dir_refs_params: the caller's bit counts of the L0 / L1 / bi decision of a B picture with several references per list (the rule:
    include/hmme.h): dir_bits = HM's uiMbBits[3], n_refs = references of list 0 and list 1, ref_bits[l][r] = reference-index + MVP-index bits
    of list l's reference r (up to 8 per list), l1_valid_mask: bit r set = list 1's reference r may win direction 2"""
    _fields_ = [("dir_bits", C.c_uint32 * 3), ("n_refs", C.c_int * 2), ("ref_bits", (C.c_uint32 * 8) * 2), ("l1_valid_mask", C.c_uint32)]

    def __init__(self, dir_bits=(0, 0, 0), n_refs=(1, 1), ref_bits=((), ()), l1_valid_mask=None):
        rb = ((C.c_uint32 * 8) * 2)()
        for l in range(2):
            for r, v in enumerate(ref_bits[l]):
                rb[l][r] = int(v)
        mask = (1 << int(n_refs[1])) - 1 if l1_valid_mask is None else int(l1_valid_mask)
        super().__init__((C.c_uint32 * 3)(*[int(v) for v in dir_bits]), (C.c_int * 2)(*[int(v) for v in n_refs]), rb, mask)


class FrameParams(C.Structure):
    _fields_ = [("search_range", C.c_int), ("fen", C.c_int), ("bit_depth", C.c_int),
                ("ctu_first", C.c_int), ("ctu_count", C.c_int)]


def build():
    """compile libhmme.so for gfx950 (hipcc cross-compiles without a GPU)"""
    subprocess.run(["make", "-s", "-C", CSRC], check=True)


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HmmeError(f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (python __graft_entry__.py). "
                        "The engine has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i = C.c_void_p, C.c_int
    if not hasattr(L, "hmme_abi_version") or L.hmme_abi_version() != ABI_VERSION:
        raise HmmeError(f"{LIB_PATH}: ABI version {L.hmme_abi_version() if hasattr(L, 'hmme_abi_version') else '< 3'}, "
                        f"these bindings need {ABI_VERSION}: rebuild with `make -C {CSRC}`")
    L.hmme_build_id.restype = C.c_char_p
    L.hmme_create.argtypes = [i, i, C.c_uint, C.POINTER(vp)]
    L.hmme_destroy.argtypes = [vp]
    L.hmme_destroy.restype = None
    L.hmme_last_error.argtypes = [vp]
    L.hmme_last_error.restype = C.c_char_p
    L.hmme_set_error_printing.argtypes = [vp, i]
    L.hmme_set_error_printing.restype = i
    L.hmme_device_info.argtypes = [vp]
    L.hmme_device_info.restype = C.c_char_p
    L.hmme_set_lambda.argtypes = [vp, C.c_double]
    L.hmme_set_lambda_q16.argtypes = [vp, C.c_uint32]
    L.hmme_get_lambda_q16.argtypes = [vp]
    L.hmme_get_lambda_q16.restype = C.c_uint32
    L.hmme_params_ocl_compat.argtypes = [C.POINTER(SearchParams), i, i, i]
    L.hmme_params_ocl_compat.restype = None
    L.hmme_set_search_range.argtypes = [i] * 7 + [C.POINTER(i)] * 4
    L.hmme_set_search_range.restype = None
    L.hmme_slot_index.argtypes = [i, i, i, i]
    L.hmme_slot_rect.argtypes = [i] + [C.POINTER(i)] * 4
    L.hmme_search_ctu.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), vp, vp]
    L.hmme_search_ctu_w.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), C.POINTER(Weight), vp, vp]
    L.hmme_search_refine_ctu_w.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), C.POINTER(Weight), i, vp, vp, vp, vp]
    L.hmme_refine_ctu_w.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), C.POINTER(Weight), vp, i, vp, vp]
    L.hmme_search_refine_ctu.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), i, vp, vp, vp, vp]
    L.hmme_refine_ctu.argtypes = [vp, vp, i, vp, i, C.POINTER(SearchParams), vp, i, vp, vp]
    L.hmme_plane_create.argtypes = [vp, i, i, C.POINTER(vp)]
    L.hmme_plane_create_ex.argtypes = [vp, i, i, i, C.POINTER(vp)]
    L.hmme_plane_bit_depth.argtypes = [vp]
    L.hmme_plane_destroy.argtypes = [vp]
    L.hmme_plane_destroy.restype = None
    L.hmme_plane_upload_pel.argtypes = [vp, vp, i]
    L.hmme_plane_upload_u8.argtypes = [vp, vp, i]
    L.hmme_host_register.argtypes = [vp, vp, C.c_size_t]
    L.hmme_host_unregister.argtypes = [vp, vp]
    L.hmme_plane_set_device_u8.argtypes = [vp, vp, i, vp]
    L.hmme_plane_width.argtypes = [vp]
    L.hmme_plane_height.argtypes = [vp]
    L.hmme_num_ctus.argtypes = [i, i]
    L.hmme_search_frame.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp]
    L.hmme_search_frame_device.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp, vp]
    L.hmme_search_frame_multi.argtypes = [vp, vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, vp]
    L.hmme_search_frame_multi_device.argtypes = [vp, vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, vp, vp]
    L.hmme_refine_frame.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, i, vp, vp]
    L.hmme_refine_frame_multi_device.argtypes = [vp, vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, i, vp, vp, vp]
    L.hmme_test_time_search_kernel.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp, vp, i, C.POINTER(C.c_float)]
    L.hmme_search_pairs_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, vp, vp]
    L.hmme_refine_pairs_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, i, vp, vp, vp]
    L.hmme_plane_upload_async.argtypes = [vp, vp, i, i, vp]
    L.hmme_weight_check.argtypes = [i, C.POINTER(Weight), i]
    L.hmme_search_pairs_w_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), C.POINTER(Weight), vp, vp, vp, vp]
    L.hmme_refine_pairs_w_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), C.POINTER(Weight), vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_w.argtypes = [vp, vp, vp, C.POINTER(FrameParams), C.POINTER(Weight), vp, vp, vp]
    L.hmme_refine_frame_w.argtypes = [vp, vp, vp, C.POINTER(FrameParams), C.POINTER(Weight), vp, vp, i, vp, vp]
    L.hmme_test_time_weight_passes.argtypes = [vp, vp, vp, C.POINTER(Weight), vp, i, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.hmme_bipred_check.argtypes = [i, i]
    L.hmme_predict_pairs_device.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_frame.argtypes = [vp, vp, C.POINTER(FrameParams), vp, i, vp, i]
    L.hmme_search_pairs_bi_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, i, vp, vp, vp, vp, vp]
    L.hmme_refine_pairs_bi_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, i, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), vp, i, vp, vp, vp, vp]
    L.hmme_refine_frame_bi.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), vp, i, vp, vp, vp, i, vp, vp]
    pw = C.POINTER(Weight)
    L.hmme_bipred_weight_check.argtypes = [i, pw, pw, i]
    L.hmme_predict_pairs_w_device.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), pw, vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_frame_w.argtypes = [vp, vp, C.POINTER(FrameParams), pw, vp, i, vp, i]
    L.hmme_search_pairs_bi_w_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), pw, pw, vp, i, vp, vp, vp, vp, vp]
    L.hmme_refine_pairs_bi_w_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), pw, pw, vp, i, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi_w.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), pw, pw, vp, i, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_w.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), pw, pw, vp, i, vp, vp, vp, i, vp, vp]
    L.hmme_test_time_bipred_origin.argtypes = [vp, vp, vp, vp, i, vp, i, C.POINTER(C.c_float)]
    L.hmme_slot_key.argtypes = [i] + [C.POINTER(i)] * 4
    L.hmme_select_check.argtypes = [C.POINTER(SelectParams)]
    L.hmme_select_pairs_device.argtypes = [vp, i, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), vp, vp, vp, vp, vp, vp, vp]
    L.hmme_select_frame.argtypes = [vp, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), vp, vp, vp, vp, vp, vp]
    L.hmme_ref_idx_bits.argtypes = [i, i]
    L.hmme_select_refs_check.argtypes = [C.POINTER(SelectParams), i, i, vp]
    L.hmme_select_refs_device.argtypes = [vp, i, i, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hmme_select_refs_frame.argtypes = [vp, i, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), vp, vp, vp, vp, vp, vp, vp, vp]
    L.hmme_predict_refs_device.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, i, vp, i, vp]
    L.hmme_predict_refs_frame.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, i, vp, i]
    L.hmme_select_dirs_check.argtypes = [C.POINTER(SelectParams), i, C.POINTER(DirParams)]
    L.hmme_select_dirs_device.argtypes = [vp, i, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), C.POINTER(DirParams)] + [vp] * 11
    L.hmme_select_dirs_frame.argtypes = [vp, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), C.POINTER(DirParams)] + [vp] * 10
    L.hmme_predict_bi_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_bi_frame.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, i, vp, i]
    L.hmme_predict_bi_weight_check.argtypes = [i, pw, pw]
    L.hmme_predict_bi_w_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), pw, pw, vp, vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_bi_w_frame.argtypes = [vp, vp, vp, C.POINTER(FrameParams), pw, pw, vp, vp, i, vp, i]
    L.hmme_predict_refs_w_device.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), pw, vp, vp, i, vp, i, vp]
    L.hmme_predict_refs_w_frame.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), pw, vp, vp, i, vp, i]
    L.hmme_predict_chroma_pairs_device.argtypes = [vp, C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_chroma_frame.argtypes = [vp, C.POINTER(vp), i, i, C.POINTER(FrameParams), pw, vp, i, C.POINTER(vp), i]
    L.hmme_predict_chroma_refs_device.argtypes = [vp, C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, vp, vp, i, vp, vp, i, vp]
    L.hmme_predict_chroma_refs_frame.argtypes = [vp, C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, vp, vp, i, C.POINTER(vp), i]
    L.hmme_predict_refs4_device.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), pw, vp, vp, vp, i, vp]
    L.hmme_predict_refs4_frame.argtypes = [vp, C.POINTER(vp), i, C.POINTER(FrameParams), pw, vp, vp, vp, i]
    L.hmme_predict_chroma_refs4_device.argtypes = [vp, C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, vp, vp, vp, vp, i, vp]
    L.hmme_predict_chroma_refs4_frame.argtypes = [vp, C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, vp, vp, C.POINTER(vp), i]
    # B pictures from one MV per 4x4 block: the bi, dirs and predict_bi signatures without mv_per_ctu (chroma: without weights, too)
    L.hmme_search_pairs_bi4_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, vp, vp, vp, vp]
    L.hmme_refine_pairs_bi4_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi4.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp, vp, vp]
    L.hmme_refine_frame_bi4.argtypes = [vp, vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp, vp, i, vp, vp]
    L.hmme_select_dirs4_check.argtypes = [C.POINTER(SelectParams), i, C.POINTER(DirParams)]
    L.hmme_select_dirs4_device.argtypes = [vp, i, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), C.POINTER(DirParams)] + [vp] * 11
    L.hmme_select_dirs4_frame.argtypes = [vp, i, i, C.POINTER(FrameParams), C.POINTER(SelectParams), C.POINTER(DirParams)] + [vp] * 10
    L.hmme_predict_bi4_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(FrameParams), vp, vp, C.POINTER(vp), i, vp]
    L.hmme_predict_bi4_frame.argtypes = [vp, vp, vp, C.POINTER(FrameParams), vp, vp, vp, i]
    L.hmme_predict_chroma_bi4_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, C.POINTER(FrameParams), vp, vp, C.POINTER(vp), i, vp]
    L.hmme_predict_chroma_bi4_frame.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(FrameParams), vp, vp, C.POINTER(vp), i]
    L.hmme_predict_chroma_bi_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, C.POINTER(FrameParams), pw, pw, vp, vp, i, C.POINTER(vp), i, vp]
    L.hmme_predict_chroma_bi_frame.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(FrameParams), pw, pw, vp, vp, i, C.POINTER(vp), i]
    L.hmme_residual_pairs_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(FrameParams), vp, i, i, C.POINTER(vp), i, vp, vp, vp, vp]
    L.hmme_residual_frame.argtypes = [vp, vp, C.POINTER(FrameParams), vp, i, vp, i, i, vp, i, vp, vp, vp]
    pvp, pfp = C.POINTER(vp), C.POINTER(FrameParams)
    L.hmme_search_frame_bi_refs_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, i, vp, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, i, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi_refs.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, i, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, i, vp, vp, vp, i, vp, vp]
    L.hmme_select_dirs_refs_check.argtypes = [C.POINTER(SelectParams), i, i, C.POINTER(DirRefsParams)]
    L.hmme_select_dirs_refs_device.argtypes = [vp, i, i, i, i, pfp, C.POINTER(SelectParams), C.POINTER(DirRefsParams)] + [vp] * 13
    L.hmme_select_dirs_refs_frame.argtypes = [vp, i, i, i, pfp, C.POINTER(SelectParams), C.POINTER(DirRefsParams)] + [vp] * 12
    L.hmme_predict_bi_refs_device.argtypes = [vp, pvp, i, pvp, i, pfp, vp, vp, vp, i, vp, i, vp]
    L.hmme_predict_bi_refs_frame.argtypes = [vp, pvp, i, pvp, i, pfp, vp, vp, vp, i, vp, i]
    # ... from one MV per 4x4 block: the bi_refs signatures without mv_per_ctu (chroma: without weights, too)
    L.hmme_search_frame_bi_refs4_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs4_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi_refs4.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs4.argtypes = [vp, vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, vp, i, vp, vp]
    L.hmme_select_dirs_refs4_check.argtypes = [C.POINTER(SelectParams), i, i, C.POINTER(DirRefsParams)]
    L.hmme_select_dirs_refs4_device.argtypes = [vp, i, i, i, i, pfp, C.POINTER(SelectParams), C.POINTER(DirRefsParams)] + [vp] * 13
    L.hmme_select_dirs_refs4_frame.argtypes = [vp, i, i, i, pfp, C.POINTER(SelectParams), C.POINTER(DirRefsParams)] + [vp] * 12
    L.hmme_predict_bi_refs4_device.argtypes = [vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, i, vp]
    L.hmme_predict_bi_refs4_frame.argtypes = [vp, pvp, i, pvp, i, pfp, vp, vp, vp, vp, i]
    L.hmme_predict_chroma_bi_refs4_device.argtypes = [vp, pvp, i, pvp, i, i, i, pfp, vp, vp, vp, vp, vp, i, vp]
    L.hmme_predict_chroma_bi_refs4_frame.argtypes = [vp, pvp, i, pvp, i, i, i, pfp, vp, vp, vp, pvp, i]
    L.hmme_bipred_refs_weight_check.argtypes = [i, pw, i, pw, i, i]
    L.hmme_search_frame_bi_refs_w_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, i, vp, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs_w_device.argtypes = [vp, vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, i, vp, vp, vp, i, vp, vp, vp]
    L.hmme_search_frame_bi_refs_w.argtypes = [vp, vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, i, vp, vp, vp, vp]
    L.hmme_refine_frame_bi_refs_w.argtypes = [vp, vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, i, vp, vp, vp, i, vp, vp]
    L.hmme_predict_bi_refs_weight_check.argtypes = [i, pw, i, pw, i]
    L.hmme_predict_bi_refs_w_device.argtypes = [vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, vp, i, vp, i, vp]
    L.hmme_predict_bi_refs_w_frame.argtypes = [vp, pvp, i, pvp, i, pfp, pw, pw, vp, vp, vp, i, vp, i]
    L.hmme_predict_chroma_bi_refs_device.argtypes = [vp, pvp, i, pvp, i, i, i, pfp, pw, pw, vp, vp, vp, i, vp, vp, i, vp]
    L.hmme_predict_chroma_bi_refs_frame.argtypes = [vp, pvp, i, pvp, i, i, i, pfp, pw, pw, vp, vp, vp, i, pvp, i]
    L.hmme_plane_stats.argtypes =[vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.hmme_wp_estimate.argtypes = [vp, vp, C.POINTER(vp), i, i, C.POINTER(Weight), C.POINTER(WpInfo)]
    L.hmme_wp_estimate_420.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(Weight), C.POINTER(Weight), C.POINTER(WpInfo)]
    L.hmme_test_time_wp_estimate_passes.argtypes = [vp, vp, C.POINTER(vp), i, C.POINTER(Weight), vp, i, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.hmme_upload_status.argtypes = [vp, vp]
    L.hmme_test_device_address.argtypes = [vp, vp]
    L.hmme_test_device_address.restype = C.c_uint64
    _lib = L
    return L


class Plane:
    def __init__(self, engine, width, height, bit_depth=8):
        self.engine = engine
        self.width, self.height, self.bit_depth = width, height, bit_depth
        h = C.c_void_p()
        engine._check(engine.L.hmme_plane_create_ex(engine.h, width, height, bit_depth, C.byref(h)))
        self.h = h

    def upload_pel(self, padded, origin):
        """padded: 2-D int16 HM plane, origin = (x, y) of sample (0,0) inside it"""
        a = np.ascontiguousarray(padded, dtype=np.int16)
        ptr = a.ctypes.data + 2 * (origin[1] * a.shape[1] + origin[0])
        self.engine._check(self.engine.L.hmme_plane_upload_pel(self.h, ptr, a.shape[1]))

    def upload_u8(self, img):
        a = np.ascontiguousarray(img, dtype=np.uint8)
        assert a.shape == (self.height, self.width)
        self.engine._check(self.engine.L.hmme_plane_upload_u8(self.h, a.ctypes.data, a.shape[1]))

    def upload_async(self, host_ptr, stride, sample_bytes, stream):
        """asynchronous upload from (page-locked) host memory on `stream`; host_ptr: address of sample (0,0)"""
        self.engine._check(self.engine.L.hmme_plane_upload_async(self.h, host_ptr, stride, sample_bytes, stream))

    @property
    def device_address(self):
        return int(self.engine.L.hmme_test_device_address(self.engine.h, self.h))

    def set_device_u8(self, dptr, pitch, stream=0):
        self.engine._check(self.engine.L.hmme_plane_set_device_u8(self.h, dptr, pitch, stream))

    def close(self):
        if self.h:
            self.engine.L.hmme_plane_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Engine:
    """one context = one GPU (reference: one TEncOpenCL object, TEncTop.h:82)"""

    def __init__(self, device=0, sr_max=64):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.hmme_create(device, sr_max, 0, C.byref(h))
        if rc != 0:
            raise HmmeError(f"hmme_create failed ({rc}): {self.L.hmme_last_error(None).decode()}")
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise HmmeError(f"hmme error {rc}: {self.L.hmme_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.hmme_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def device_info(self):
        return self.L.hmme_device_info(self.h).decode()

    def set_lambda(self, lam):
        self._check(self.L.hmme_set_lambda(self.h, float(lam)))

    def set_lambda_q16(self, q):
        """any uint32 (the MV cost's product wraps in 32 bits, as HM's); ValueError outside 0..2^32-1, which ctypes would truncate silently"""
        if not 0 <= int(q) <= 0xFFFFFFFF:
            raise ValueError(f"lambda_q16 {q} is outside 0..2^32-1")
        self._check(self.L.hmme_set_lambda_q16(self.h, int(q)))

    @property
    def lambda_q16(self):
        return int(self.L.hmme_get_lambda_q16(self.h))

    def plane(self, width, height, bit_depth=8):
        return Plane(self, width, height, bit_depth)

    def host_register(self, array):
        """page-lock a long-lived numpy buffer: uploads from it then run at PCIe rate (hmme_host_register)"""
        self._check(self.L.hmme_host_register(self.h, array.ctypes.data, array.nbytes))

    def host_unregister(self, array):
        self._check(self.L.hmme_host_unregister(self.h, array.ctypes.data))

    def _ctu(self, fn, cur_plane, cur_xy, ref_plane, ref_xy, params, wp=None, int_mv=None, use_hadamard=None):
        """the six per-CTU entries.  planes: 2-D int16; *_xy = CTU origin inside them; wp = (w0, offset, shift, round) for a _w entry;
        int_mv: the caller's integer MVs instead of a search; use_hadamard given: the entry refines.
        -> the tables of the search (mv int16[593,2], sad uint32[593]), then those of the refinement (qmv int16[593,2] quarter-pel, cost uint32[593])"""
        cur = np.ascontiguousarray(cur_plane, dtype=np.int16)
        ref = np.ascontiguousarray(ref_plane, dtype=np.int16)
        args = [self.h, cur.ctypes.data + 2 * (cur_xy[1] * cur.shape[1] + cur_xy[0]), cur.shape[1],
                ref.ctypes.data + 2 * (ref_xy[1] * ref.shape[1] + ref_xy[0]), ref.shape[1], C.byref(params)]
        if wp is not None:
            w = Weight(*[int(v) for v in wp])
            args.append(C.byref(w))
        if int_mv is not None:
            imv = np.ascontiguousarray(int_mv, dtype=np.int16)
            assert imv.shape == (NUM_PARTS, 2)
            args.append(imv.ctypes.data)
        if use_hadamard is not None:
            args.append(1 if use_hadamard else 0)
        tables = (int_mv is None) + (use_hadamard is not None)   # a pair of arrays each for the search and the refinement
        outs = [a for _ in range(tables) for a in (np.zeros((NUM_PARTS, 2), np.int16), np.zeros(NUM_PARTS, np.uint32))]
        self._check(fn(*args, *[o.ctypes.data for o in outs]))
        return tuple(outs)

    def search_ctu(self, cur_plane, cur_xy, ref_plane, ref_xy, params):
        """per-CTU drop-in (calcMotionVectors) -> (mv, sad)"""
        return self._ctu(self.L.hmme_search_ctu, cur_plane, cur_xy, ref_plane, ref_xy, params)

    def search_ctu_w(self, cur_plane, cur_xy, ref_plane, ref_xy, params, wp):
        """hmme_search_ctu_w: the per-CTU search of a slice with explicit weighted prediction -> (mv, sad)"""
        return self._ctu(self.L.hmme_search_ctu_w, cur_plane, cur_xy, ref_plane, ref_xy, params, wp=wp)

    def search_refine_ctu_w(self, cur_plane, cur_xy, ref_plane, ref_xy, params, wp, use_hadamard=True):
        """hmme_search_refine_ctu_w: weighted integer search + weighted xPatternSearchFracDIF in one call -> (mv, sad, qmv, cost)"""
        return self._ctu(self.L.hmme_search_refine_ctu_w, cur_plane, cur_xy, ref_plane, ref_xy, params, wp=wp, use_hadamard=bool(use_hadamard))

    def search_refine_ctu(self, cur_plane, cur_xy, ref_plane, ref_xy, params, use_hadamard=True):
        """hmme_search_ctu + xPatternSearchFracDIF of its winners in one call -> (mv, sad, qmv, cost)"""
        return self._ctu(self.L.hmme_search_refine_ctu, cur_plane, cur_xy, ref_plane, ref_xy, params, use_hadamard=bool(use_hadamard))

    def refine_ctu(self, cur_plane, cur_xy, ref_plane, ref_xy, params, int_mv, use_hadamard=True):
        """xPatternSearchFracDIF for the 593 slots of one CTU at the caller's integer MVs -> (qmv, cost)"""
        return self._ctu(self.L.hmme_refine_ctu, cur_plane, cur_xy, ref_plane, ref_xy, params, int_mv=int_mv, use_hadamard=bool(use_hadamard))

    def refine_ctu_w(self, cur_plane, cur_xy, ref_plane, ref_xy, params, wp, int_mv, use_hadamard=True):
        """hmme_refine_ctu_w: the weighted xPatternSearchFracDIF alone, at the caller's integer MVs -> (qmv, cost)"""
        return self._ctu(self.L.hmme_refine_ctu_w, cur_plane, cur_xy, ref_plane, ref_xy, params, wp=wp, int_mv=int_mv, use_hadamard=bool(use_hadamard))


    def search_frame(self, cur, ref, sr, pred_q=None, fen=1, bit_depth=None, ctu_first=0, ctu_count=-1):
        """-> (mv int16[count,593,2], sad uint32[count,593])"""
        bit_depth = cur.bit_depth if bit_depth is None else bit_depth
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), bit_depth, ctu_first, count)
        mv = np.zeros((count, NUM_PARTS, 2), np.int16)
        sad = np.zeros((count, NUM_PARTS), np.uint32)
        pq = None
        if pred_q is not None:
            pred_q = np.ascontiguousarray(pred_q, dtype=np.int16)
            assert pred_q.shape == (n, 2)
            pq = pred_q.ctypes.data
        self._check(self.L.hmme_search_frame(self.h, cur.h, ref.h, C.byref(fp), pq, mv.ctypes.data, sad.ctypes.data))
        return mv, sad

    def search_frame_multi(self, cur, refs, sr, pred_q=None, fen=1, ctu_first=0, ctu_count=-1):
        """several reference pictures in one launch -> (mv int16[n_refs,count,593,2], sad uint32[n_refs,count,593])"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        mv = np.zeros((len(refs), count, NUM_PARTS, 2), np.int16)
        sad = np.zeros((len(refs), count, NUM_PARTS), np.uint32)
        pq = None
        if pred_q is not None:
            pred_q = np.ascontiguousarray(pred_q, dtype=np.int16)
            assert pred_q.shape == (len(refs), n, 2)
            pq = pred_q.ctypes.data
        arr = _handles(refs)
        self._check(self.L.hmme_search_frame_multi(self.h, cur.h, arr, len(refs), C.byref(fp), pq, mv.ctypes.data, sad.ctypes.data))
        return mv, sad

    def refine_frame(self, cur, ref, sr, int_mv, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """fractional-pel refinement of integer winners -> (qmv int16[count,593,2] quarter-pel, cost uint32[count,593])"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, 1, cur.bit_depth, ctu_first, count)
        int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
        assert int_mv.shape == (count, NUM_PARTS, 2)
        qmv = np.zeros((count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((count, NUM_PARTS), np.uint32)
        pq = None
        if pred_q is not None:
            pred_q = np.ascontiguousarray(pred_q, dtype=np.int16)
            pq = pred_q.ctypes.data
        self._check(self.L.hmme_refine_frame(self.h, cur.h, ref.h, C.byref(fp), pq, int_mv.ctypes.data, int(use_hadamard),
                                             qmv.ctypes.data, cost.ctypes.data))
        return qmv, cost

    def refine_frame_multi_device(self, cur, refs, fp, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        arr = _handles(refs)
        self._check(self.L.hmme_refine_frame_multi_device(self.h, cur.h, arr, len(refs), C.byref(fp), d_pred, d_int_mv,
                                                          int(use_hadamard), d_qmv, d_cost, stream))

    def search_frame_multi_device(self, cur, refs, fp, d_pred, d_mv, d_sad, stream=0):
        arr = _handles(refs)
        self._check(self.L.hmme_search_frame_multi_device(self.h, cur.h, arr, len(refs), C.byref(fp), d_pred, d_mv, d_sad, stream))

    def search_pairs_device(self, curs, refs, fp, d_pred, d_mv, d_sad, stream=0):
        """up to 16 (current, reference) picture pairs of one size in one launch (hmme_search_pairs_device)"""
        assert len(curs) == len(refs)
        ca = _handles(curs)
        ra = _handles(refs)
        self._check(self.L.hmme_search_pairs_device(self.h, ca, ra, len(refs), C.byref(fp), d_pred, d_mv, d_sad, stream))

    def refine_pairs_device(self, curs, refs, fp, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        assert len(curs) == len(refs)
        ca = _handles(curs)
        ra = _handles(refs)
        self._check(self.L.hmme_refine_pairs_device(self.h, ca, ra, len(refs), C.byref(fp), d_pred, d_int_mv, int(use_hadamard),
                                                    d_qmv, d_cost, stream))

    def search_frame_w(self, cur, ref, sr, wp, pred_q=None, fen=0, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_w: the whole-picture search of a slice with explicit weighted prediction, wp = (w0, offset, shift, round)
        (fen is passed through and not consulted by the engine) -> (mv int16[count,593,2], sad uint32[count,593])"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        mv = np.zeros((count, NUM_PARTS, 2), np.int16)
        sad = np.zeros((count, NUM_PARTS), np.uint32)
        pq = None
        if pred_q is not None:
            pred_q = np.ascontiguousarray(pred_q, dtype=np.int16)
            assert pred_q.shape == (n, 2)
            pq = pred_q.ctypes.data
        w = Weight(*[int(v) for v in wp])
        self._check(self.L.hmme_search_frame_w(self.h, cur.h, ref.h, C.byref(fp), C.byref(w), pq, mv.ctypes.data, sad.ctypes.data))
        return mv, sad

    def refine_frame_w(self, cur, ref, sr, wp, int_mv, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_w: weighted xPatternSearchFracDIF of integer winners -> (qmv int16[count,593,2], cost uint32[count,593])"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, 0, cur.bit_depth, ctu_first, count)
        int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
        assert int_mv.shape == (count, NUM_PARTS, 2)
        qmv = np.zeros((count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((count, NUM_PARTS), np.uint32)
        pq = None
        if pred_q is not None:
            pred_q = np.ascontiguousarray(pred_q, dtype=np.int16)
            assert pred_q.shape == (n, 2)
            pq = pred_q.ctypes.data
        w = Weight(*[int(v) for v in wp])
        self._check(self.L.hmme_refine_frame_w(self.h, cur.h, ref.h, C.byref(fp), C.byref(w), pq, int_mv.ctypes.data, int(use_hadamard),
                                               qmv.ctypes.data, cost.ctypes.data))
        return qmv, cost

    def search_pairs_w_device(self, curs, refs, fp, weights, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_pairs_w_device: up to 16 pairs in one launch, weights = one (w0, offset, shift, round) per pair"""
        assert len(curs) == len(refs) == len(weights)
        ca = _handles(curs)
        ra = _handles(refs)
        wa = (Weight * len(weights))(*[Weight(*[int(v) for v in w]) for w in weights])
        self._check(self.L.hmme_search_pairs_w_device(self.h, ca, ra, len(refs), C.byref(fp), wa, d_pred, d_mv, d_sad, stream))

    def refine_pairs_w_device(self, curs, refs, fp, weights, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        assert len(curs) == len(refs) == len(weights)
        ca = _handles(curs)
        ra = _handles(refs)
        wa = (Weight * len(weights))(*[Weight(*[int(v) for v in w]) for w in weights])
        self._check(self.L.hmme_refine_pairs_w_device(self.h, ca, ra, len(refs), C.byref(fp), wa, d_pred, d_int_mv, int(use_hadamard),
                                                      d_qmv, d_cost, stream))

    def time_weight_passes(self, cur, ref, wp, stream=0, reps=5):
        """device time in ms of the two plane passes of a weighted search on their own -> (reference plane, current-picture blocks)"""
        a, b = C.c_float(), C.c_float()
        w = Weight(*[int(v) for v in wp])
        self._check(self.L.hmme_test_time_weight_passes(self.h, cur.h, ref.h, C.byref(w), stream, reps, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- motion compensation and the bi-prediction pass on whole pictures (include/hmme.h, "bi-prediction on whole pictures") ----
    @staticmethod
    def _field(mv_field, n_ctu):
        """a host motion field int16[n_ctu, mv_per_ctu, 2] (or [n_ctu, 2]: one MV per CTU) -> (contiguous array, mv_per_ctu)"""
        f = np.ascontiguousarray(mv_field, dtype=np.int16)
        if f.ndim == 2:
            f = f.reshape(f.shape[0], 1, 2)
        assert f.shape[0] == n_ctu and f.shape[1] in (1, 64) and f.shape[2] == 2
        return f, int(f.shape[1])

    @staticmethod
    def _pq(a, n_ctu):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.int16)
        assert a.shape == (n_ctu, 2)
        return a, a.ctypes.data

    @staticmethod
    def _image(ref, out):
        """the image argument of the predict_* methods: `out`, or zeros when None, of the plane's size and sample type"""
        dt = np.uint8 if ref.bit_depth == 8 else np.uint16
        if out is None:
            out = np.zeros((ref.height, ref.width), dt)
        assert out.dtype == dt and out.shape == (ref.height, ref.width) and out.flags.c_contiguous
        return out

    def _predict_fields(self, plane, width, height, mv_field, block_field, lists, ctu_first, ctu_count):
        """what the predict_*_frame methods prepare alike, for a picture of width x height LUMA samples whose planes are like `plane`: the
        motion field (lists == 2: the two lists' fields, stacked), the reference / direction field beside it (None: the form has none) and the
        call's parameters -> (field, mv_per_ctu, block field or None, FrameParams)"""
        n = self.L.hmme_num_ctus(int(width), int(height))
        if lists == 1:
            f, per = self._field(mv_field, n)
        else:
            f0, per = self._field(mv_field[0], n)
            f1, per1 = self._field(mv_field[1], n)
            assert per == per1
            f = np.ascontiguousarray(np.stack([f0, f1]))
        bf = None
        if block_field is not None:
            bf = np.ascontiguousarray(block_field, dtype=np.uint8).reshape(n, -1)
            assert bf.shape == (n, per)
        return f, per, bf, FrameParams(1, 0, plane.bit_depth, ctu_first, ctu_count)

    def predict_pairs_device(self, refs, fp, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_pairs_device: the luma prediction of up to 16 pictures from their motion fields; d_outs = one device image address per picture"""
        assert len(refs) == len(d_outs)
        ra = _handles(refs)
        oa = (C.c_void_p * len(d_outs))(*[int(o) for o in d_outs])
        self._check(self.L.hmme_predict_pairs_device(self.h, ra, len(refs), C.byref(fp), d_mv_field, int(mv_per_ctu), oa, int(out_pitch_bytes), stream))

    def predict_frame(self, ref, mv_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_frame: motion-compensated luma prediction of one picture -> [height, width] array of the plane's sample type (u8 / u16).
        mv_field: int16[n_ctu, 2] or [n_ctu, 1 | 64, 2] quarter pels; `out` (same shape and type) keeps its samples outside the CTU range"""
        f, per, _, fp = self._predict_fields(ref, ref.width, ref.height, mv_field, None, 1, ctu_first, ctu_count)
        out = self._image(ref, out)
        self._check(self.L.hmme_predict_frame(self.h, ref.h, C.byref(fp), f.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    def search_pairs_bi_device(self, curs, refs, others, fp, d_other_mv, mv_per_ctu, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_pairs_bi_device: the bi-prediction pass of up to 16 pairs in one launch (origin 2 * cur - prediction of others[i])"""
        assert len(curs) == len(refs) == len(others)
        ca = _handles(curs)
        ra = _handles(refs)
        oa = _handles(others)
        self._check(self.L.hmme_search_pairs_bi_device(self.h, ca, ra, oa, len(refs), C.byref(fp), d_other_mv, int(mv_per_ctu), d_center, d_pred,
                                                       d_mv, d_sad, stream))

    def refine_pairs_bi_device(self, curs, refs, others, fp, d_other_mv, mv_per_ctu, d_center, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        assert len(curs) == len(refs) == len(others)
        ca = _handles(curs)
        ra = _handles(refs)
        oa = _handles(others)
        self._check(self.L.hmme_refine_pairs_bi_device(self.h, ca, ra, oa, len(refs), C.byref(fp), d_other_mv, int(mv_per_ctu), d_center, d_pred,
                                                       d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def _frame_bi(self, entry, cur, ref, other, sr, fen, weights, other_mv, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count):
        """the four *_frame_bi* methods: weights = (wp, other_wp) for the *_w entries, else (); int_mv: None for a search -> the two result tables"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        f, per = self._field(other_mv, n)
        cq, cptr = self._pq(center_q, n)
        pq, pptr = self._pq(pred_q, n)
        args = [C.byref(Weight(*[int(v) for v in w])) for w in weights] + [f.ctypes.data, per, cptr, pptr]
        if int_mv is not None:
            int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
            assert int_mv.shape == (count, NUM_PARTS, 2)
            args += [int_mv.ctypes.data, int(use_hadamard)]
        mv = np.zeros((count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((count, NUM_PARTS), np.uint32)
        self._check(entry(self.h, cur.h, ref.h, other.h, C.byref(fp), *args, mv.ctypes.data, cost.ctypes.data))
        return mv, cost

    def search_frame_bi(self, cur, ref, other, sr, other_mv, center_q=None, pred_q=None, fen=1, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi: one pair, host arrays -> (mv int16[count,593,2], sad uint32[count,593]).  other_mv: the motion field of `other`
        (int16[n_ctu, 2] or [n_ctu, 1 | 64, 2]); center_q: window centres int16[n_ctu, 2] (None: the predictors)"""
        return self._frame_bi(self.L.hmme_search_frame_bi, cur, ref, other, sr, fen, (), other_mv, None, center_q, pred_q, True, ctu_first, ctu_count)

    def refine_frame_bi(self, cur, ref, other, sr, other_mv, int_mv, center_q=None, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi: xPatternSearchFracDIF of integer winners against the bi-prediction origin -> (qmv int16[count,593,2], cost uint32[count,593])"""
        return self._frame_bi(self.L.hmme_refine_frame_bi, cur, ref, other, sr, 1, (), other_mv, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count)

    # ---- ... in a slice with explicit weighted prediction (include/hmme.h, "bi-prediction with explicit weighted prediction"): weights are
    # (w0, offset, shift, round); `wp` / `weights` belong to the searched list, `other_wp` / `other_weights` to the list whose prediction is subtracted
    @staticmethod
    def _weights(weights):
        return (Weight * len(weights))(*[Weight(*[int(v) for v in w]) for w in weights])

    def predict_pairs_w_device(self, refs, fp, weights, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_pairs_w_device: predict_pairs_device with one weight per picture (the prediction HM's motionCompensation writes in a WP slice)"""
        assert len(refs) == len(d_outs) == len(weights)
        ra = _handles(refs)
        oa = (C.c_void_p * len(d_outs))(*[int(o) for o in d_outs])
        self._check(self.L.hmme_predict_pairs_w_device(self.h, ra, len(refs), C.byref(fp), self._weights(weights), d_mv_field, int(mv_per_ctu), oa,
                                                       int(out_pitch_bytes), stream))

    def predict_frame_w(self, ref, wp, mv_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_frame_w: predict_frame with the weight wp"""
        f, per, _, fp = self._predict_fields(ref, ref.width, ref.height, mv_field, None, 1, ctu_first, ctu_count)
        out = self._image(ref, out)
        w = Weight(*[int(v) for v in wp])
        self._check(self.L.hmme_predict_frame_w(self.h, ref.h, C.byref(fp), C.byref(w), f.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    def search_pairs_bi_w_device(self, curs, refs, others, fp, weights, other_weights, d_other_mv, mv_per_ctu, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_pairs_bi_w_device: the bi-prediction pass of up to 16 pairs of a WP slice in one launch"""
        assert len(curs) == len(refs) == len(others) == len(weights) == len(other_weights)
        ca = _handles(curs)
        ra = _handles(refs)
        oa = _handles(others)
        self._check(self.L.hmme_search_pairs_bi_w_device(self.h, ca, ra, oa, len(refs), C.byref(fp), self._weights(weights), self._weights(other_weights),
                                                         d_other_mv, int(mv_per_ctu), d_center, d_pred, d_mv, d_sad, stream))

    def refine_pairs_bi_w_device(self, curs, refs, others, fp, weights, other_weights, d_other_mv, mv_per_ctu, d_center, d_pred, d_int_mv, use_hadamard,
                                 d_qmv, d_cost, stream=0):
        assert len(curs) == len(refs) == len(others) == len(weights) == len(other_weights)
        ca = _handles(curs)
        ra = _handles(refs)
        oa = _handles(others)
        self._check(self.L.hmme_refine_pairs_bi_w_device(self.h, ca, ra, oa, len(refs), C.byref(fp), self._weights(weights), self._weights(other_weights),
                                                         d_other_mv, int(mv_per_ctu), d_center, d_pred, d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def search_frame_bi_w(self, cur, ref, other, sr, wp, other_wp, other_mv, center_q=None, pred_q=None, fen=0, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi_w: search_frame_bi in a WP slice (fen is passed through and not consulted by the engine)
        -> (mv int16[count,593,2], sad uint32[count,593])"""
        return self._frame_bi(self.L.hmme_search_frame_bi_w, cur, ref, other, sr, fen, (wp, other_wp), other_mv, None, center_q, pred_q, True, ctu_first, ctu_count)

    def refine_frame_bi_w(self, cur, ref, other, sr, wp, other_wp, other_mv, int_mv, center_q=None, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi_w: refine_frame_bi in a WP slice -> (qmv int16[count,593,2], cost uint32[count,593])"""
        return self._frame_bi(self.L.hmme_refine_frame_bi_w, cur, ref, other, sr, 0, (wp, other_wp), other_mv, int_mv, center_q, pred_q, use_hadamard, ctu_first,
                              ctu_count)

    # ---- partition decision and motion field from the 593-slot tables (include/hmme.h, "partition decision and motion field") ----
    def select_pairs_device(self, width, height, n_pairs, fp, sel, d_mv, d_cost, d_pred, d_field, d_slot=None, d_ctu_cost=None, stream=0):
        """hmme_select_pairs_device: the tables of up to 16 pairs (device, as a search / refinement with the same fp wrote them) -> motion field
        int16[n_pairs, n_ctu, mv_per_ctu, 2], covering slots uint16[n_pairs, n_ctu, mv_per_ctu] and CTU costs uint32[n_pairs, n_ctu] (device
        addresses; d_slot / d_ctu_cost may be None)"""
        self._check(self.L.hmme_select_pairs_device(self.h, int(width), int(height), int(n_pairs), C.byref(fp), C.byref(sel), d_mv, d_cost, d_pred,
                                                    d_field, d_slot, d_ctu_cost, stream))

    def _select_frame(self, call, lead, width, height, tables, inputs, pred_q, ctu_first, ctu_count, outs):
        """the four select_*frame methods.  lead: the dimensions the tables and pred_q carry in front -- (), (n_refs,), (2,), (2, R); tables: the MV
        (int16, [*lead, count, 593, 2]) and cost (uint32, [*lead, count, 593]) tables in the entry's order; inputs: (array, dtype, lead, shape
        behind n_ctu) per further input; pred_q int16[*lead, n_ctu, 2] or None; outs: (array or None, dtype, lead, shape behind n_ctu) per output.
        call(fp, *addresses in that order) -> the C entry's return code.  -> the outputs, zeros where None was passed"""
        n = self.L.hmme_num_ctus(width, height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(1, 0, 8, ctu_first, count)
        ins = []
        for k, a in enumerate(tables):                                           # MV and cost tables alternate
            a = np.ascontiguousarray(a, dtype=np.uint32 if k % 2 else np.int16)
            assert a.shape == lead + (count, NUM_PARTS) + (() if k % 2 else (2,))
            ins.append(a)
        for a, dt, front, shape in inputs:
            a = np.ascontiguousarray(a, dtype=dt)
            assert a.shape == front + (n,) + shape
            ins.append(a)
        pptr = None
        if pred_q is not None:
            pq = np.ascontiguousarray(pred_q, dtype=np.int16)
            assert pq.shape == lead + (n, 2)
            pptr = pq.ctypes.data
        arrays = []
        for a, dt, front, shape in outs:
            a = np.zeros(front + (n,) + shape, dt) if a is None else a
            assert a.dtype == dt and a.shape == front + (n,) + shape and a.flags.c_contiguous
            arrays.append(a)
        self._check(call(fp, *[a.ctypes.data for a in ins], pptr, *[a.ctypes.data for a in arrays]))
        return tuple(arrays)

    def select_frame(self, width, height, sel, mv, cost, pred_q=None, ctu_first=0, ctu_count=-1, field=None, slot=None, ctu_cost=None):
        """hmme_select_frame: one pair, host arrays.  mv int16[count, 593, 2], cost uint32[count, 593] -> (field int16[n_ctu, mv_per_ctu, 2],
        slot uint16[n_ctu, mv_per_ctu], ctu_cost uint32[n_ctu]); entries outside the CTU range keep the values of the arrays passed in (zeros
        when none is)"""
        per = int(sel.mv_per_ctu)
        call = lambda fp, *a: self.L.hmme_select_frame(self.h, int(width), int(height), C.byref(fp), C.byref(sel), *a)
        return self._select_frame(call, (), width, height, (mv, cost), (), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (), (per, 2)), (slot, np.uint16, (), (per,)), (ctu_cost, np.uint32, (), ())))

    # ---- the reference picture per PU, and the prediction from it (include/hmme.h, "the reference picture per PU") ----
    def select_refs_device(self, width, height, n_pics, n_refs, fp, sel, ref_cost, d_mv, d_cost, d_pred, d_field, d_ref, d_slot=None, d_ctu_cost=None,
                           stream=0):
        """hmme_select_refs_device: the tables of n_pics pictures x n_refs references (device, [n_pics, n_refs, count, 593, ...] as a multi-reference
        search / refinement with the same fp wrote them) -> motion field int16[n_pics, n_ctu, mv_per_ctu, 2], reference indices uint8[n_pics, n_ctu,
        mv_per_ctu], covering slots uint16 of that shape and CTU costs uint32[n_pics, n_ctu] (device addresses; d_slot / d_ctu_cost may be None).
        ref_cost: n_refs host integers, or None for zeros"""
        self._check(self.L.hmme_select_refs_device(self.h, int(width), int(height), int(n_pics), int(n_refs), C.byref(fp), C.byref(sel),
                                                   _ref_cost(ref_cost, n_refs), d_mv, d_cost, d_pred, d_field, d_ref, d_slot, d_ctu_cost, stream))

    def select_refs_frame(self, width, height, sel, mv, cost, ref_cost=None, pred_q=None, ctu_first=0, ctu_count=-1, field=None, ref=None, slot=None,
                          ctu_cost=None):
        """hmme_select_refs_frame: one picture, host arrays.  mv int16[n_refs, count, 593, 2], cost uint32[n_refs, count, 593], pred_q
        int16[n_refs, n_ctu, 2] or None -> (field int16[n_ctu, mv_per_ctu, 2], ref uint8[n_ctu, mv_per_ctu], slot uint16[n_ctu, mv_per_ctu],
        ctu_cost uint32[n_ctu]); entries outside the CTU range keep the values of the arrays passed in (zeros when none is)"""
        per = int(sel.mv_per_ctu)
        n_refs = np.shape(mv)[0]
        call = lambda fp, *a: self.L.hmme_select_refs_frame(self.h, int(width), int(height), n_refs, C.byref(fp), C.byref(sel), _ref_cost(ref_cost, n_refs), *a)
        return self._select_frame(call, (n_refs,), width, height, (mv, cost), (), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (), (per, 2)), (ref, np.uint8, (), (per,)), (slot, np.uint16, (), (per,)), (ctu_cost, np.uint32, (), ())))

    def predict_refs_device(self, refs, fp, d_mv_field, d_ref_field, mv_per_ctu, d_out, out_pitch_bytes, stream=0):
        """hmme_predict_refs_device: the luma prediction of one picture, every block from the plane of `refs` its reference index names
        (d_ref_field uint8[n_ctu, mv_per_ctu]; blocks with an index >= len(refs) are not written); d_out = the device image"""
        ra = _handles(refs)
        self._check(self.L.hmme_predict_refs_device(self.h, ra, len(refs), C.byref(fp), d_mv_field, d_ref_field, int(mv_per_ctu), d_out,
                                                    int(out_pitch_bytes), stream))

    def predict_refs_frame(self, refs, mv_field, ref_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_refs_frame: motion-compensated luma prediction of one picture from several references -> [height, width] array of the
        planes' sample type (u8 / u16).  mv_field: int16[n_ctu, 2] or [n_ctu, 1 | 64, 2] quarter pels; ref_field: uint8[n_ctu] or [n_ctu, 1 | 64],
        the plane of `refs` per block; `out` (same shape and type) keeps its samples outside the CTU range and in blocks whose index is
        >= len(refs)"""
        r0 = refs[0]
        f, per, rf, fp = self._predict_fields(r0, r0.width, r0.height, mv_field, ref_field, 1, ctu_first, ctu_count)
        out = self._image(r0, out)
        ra = _handles(refs)
        self._check(self.L.hmme_predict_refs_frame(self.h, ra, len(refs), C.byref(fp), f.ctypes.data, rf.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    # ---- residual and distortion of a prediction (include/hmme.h, "residual and distortion of a prediction") ----
    def residual_pairs_device(self, curs, d_preds, pred_pitch_bytes, fp, d_slot, mv_per_ctu, use_hadamard, d_resids, resid_pitch_bytes, d_pu, d_cu,
                              d_ctu, stream=0):
        """hmme_residual_pairs_device: for up to 16 (current plane, predicted device image) pairs the residual images (d_resids: one int16 device
        image per pair, entries or the whole list None), the PU error and the CU SSE per block (uint32[n_pairs, n_ctu, mv_per_ctu]) and the CTU
        sums (uint32[n_pairs, n_ctu, 2]); d_slot: the covering slots uint16[n_pairs, n_ctu, mv_per_ctu] of a select call, or None (every
        block its own PU and CU).  Device addresses; d_pu / d_cu / d_ctu may be None"""
        assert len(curs) == len(d_preds) and (d_resids is None or len(d_resids) == len(curs))
        ca = _handles(curs)
        pa = (C.c_void_p * len(d_preds))(*[int(p) for p in d_preds])
        ra = None if d_resids is None else (C.c_void_p * len(d_resids))(*[None if r is None else int(r) for r in d_resids])
        self._check(self.L.hmme_residual_pairs_device(self.h, ca, pa, int(pred_pitch_bytes), len(curs), C.byref(fp), d_slot, int(mv_per_ctu),
                                                      int(use_hadamard), ra, int(resid_pitch_bytes), d_pu, d_cu, d_ctu, stream))

    def residual_frame(self, cur, pred, slot=None, mv_per_ctu=64, use_hadamard=True, ctu_first=0, ctu_count=-1, resid=None, pu=None, cu=None, ctu=None):
        """hmme_residual_frame: one picture, host arrays.  pred: [height, width] of the plane's sample type (u8 / u16); slot: uint16[n_ctu,
        mv_per_ctu] or None -> (resid int16[height, width], pu uint32[n_ctu, mv_per_ctu], cu of that shape, ctu uint32[n_ctu, 2]); samples and
        entries outside the CTU range keep the values of the arrays passed in (zeros when none is)"""
        n, per = self.L.hmme_num_ctus(cur.width, cur.height), int(mv_per_ctu)
        fp = FrameParams(1, 0, cur.bit_depth, ctu_first, ctu_count)
        pred = np.ascontiguousarray(pred, dtype=np.uint8 if cur.bit_depth == 8 else np.uint16)
        assert pred.shape == (cur.height, cur.width)
        sptr = None
        if slot is not None:
            slot = np.ascontiguousarray(slot, dtype=np.uint16)
            assert slot.shape == (n, per)
            sptr = slot.ctypes.data
        outs = []
        for a, dt, shape in ((resid, np.int16, (cur.height, cur.width)), (pu, np.uint32, (n, per)), (cu, np.uint32, (n, per)), (ctu, np.uint32, (n, 2))):
            a = np.zeros(shape, dt) if a is None else a
            assert a.dtype == dt and a.shape == shape and a.flags.c_contiguous
            outs.append(a)
        self._check(self.L.hmme_residual_frame(self.h, cur.h, C.byref(fp), pred.ctypes.data, cur.width, sptr, per, 1 if use_hadamard else 0,
                                               outs[0].ctypes.data, cur.width, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data))
        return tuple(outs)

    # ---- L0, L1 or bi per PU, and the prediction from it (include/hmme.h, "L0, L1 or bi per PU") ----
    def select_dirs_device(self, width, height, n_pics, fp, sel, dirs, d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_pred, d_field, d_dir,
                           d_slot=None, d_ctu_cost=None, stream=0):
        """hmme_select_dirs_device: the four refinement table sets of n_pics B pictures (device: uni and bi, each [n_pics, 2, count, 593, ...]) and
        the lists' uni fields int16[n_pics, 2, n_ctu, 64, 2] -> motion field of that shape, directions uint8[n_pics, n_ctu, 64] (1, 2, 3; 0xFF: no
        CU), covering slots uint16 of that shape and CTU costs uint32[n_pics, n_ctu] (device addresses; d_slot / d_ctu_cost may be None).
        dirs: one DirParams per picture"""
        self._check(self.L.hmme_select_dirs_device(self.h, int(width), int(height), int(n_pics), C.byref(fp), C.byref(sel), _dir_params(dirs, n_pics),
                                                   d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_pred, d_field, d_dir, d_slot, d_ctu_cost, stream))

    def select_dirs_frame(self, width, height, sel, dir_params, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, pred_q=None, ctu_first=0, ctu_count=-1,
                          field=None, dirs=None, slot=None, ctu_cost=None):
        """hmme_select_dirs_frame: one picture, host arrays.  mv_uni / mv_bi int16[2, count, 593, 2], cost_uni / cost_bi uint32[2, count, 593],
        uni_field int16[2, n_ctu, 64, 2], pred_q int16[2, n_ctu, 2] or None -> (field int16[2, n_ctu, 64, 2], dirs uint8[n_ctu, 64], slot
        uint16[n_ctu, 64], ctu_cost uint32[n_ctu]); entries outside the CTU range keep the values of the arrays passed in (zeros when none is)"""
        call = lambda fp, *a: self.L.hmme_select_dirs_frame(self.h, int(width), int(height), C.byref(fp), C.byref(sel), C.byref(dir_params), *a)
        return self._select_frame(call, (2,), width, height, (mv_uni, cost_uni, mv_bi, cost_bi), ((uni_field, np.int16, (2,), (64, 2)),), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (2,), (64, 2)), (dirs, np.uint8, (), (64,)), (slot, np.uint16, (), (64,)), (ctu_cost, np.uint32, (), ())))

    def predict_bi_device(self, refs0, refs1, fp, d_mv_field, d_dir_field, mv_per_ctu, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_bi_device: the luma prediction of up to 8 pictures whose blocks are L0 (refs0[i]), L1 (refs1[i]) or bi (both, averaged
        like TComYuv::addAvg): d_mv_field int16[n_pics, 2, n_ctu, mv_per_ctu, 2], d_dir_field uint8[n_pics, n_ctu, mv_per_ctu]; d_outs = one device
        image address per picture"""
        assert len(refs0) == len(refs1) == len(d_outs)
        oa = (C.c_void_p * len(d_outs))(*[int(o) for o in d_outs])
        self._check(self.L.hmme_predict_bi_device(self.h, _handles(refs0), _handles(refs1), len(refs0), C.byref(fp), d_mv_field, d_dir_field, int(mv_per_ctu),
                                                  oa, int(out_pitch_bytes), stream))

    def predict_bi_frame(self, ref0, ref1, mv_field, dir_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi_frame: the prediction of one picture from list 0 (ref0) and list 1 (ref1) -> [height, width] array of the planes'
        sample type.  mv_field: int16[2, n_ctu, 2] or [2, n_ctu, 1 | 64, 2] quarter pels; dir_field: uint8[n_ctu] or [n_ctu, 1 | 64] (1, 2, 3;
        anything else: not written); `out` keeps its samples outside the CTU range and in blocks without a direction"""
        f, per, df, fp = self._predict_fields(ref0, ref0.width, ref0.height, mv_field, dir_field, 2, ctu_first, ctu_count)
        out = self._image(ref0, out)
        self._check(self.L.hmme_predict_bi_frame(self.h, ref0.h, ref1.h, C.byref(fp), f.ctypes.data, df.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    # ---- B pictures with several references per list (include/hmme.h, "B pictures with several references per list") ----
    def search_frame_bi_refs_device(self, cur, refs, others, fp, d_other_mv, d_other_ref, mv_per_ctu, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_frame_bi_refs_device: the bi pass of one list over all its references `refs` against ONE origin, 2 * cur - the prediction
        of `others` with a motion field and a reference index per block (d_other_ref uint8[n_ctu, mv_per_ctu]; an index >= len(others) reads
        others[0]); tables [len(refs), count, 593, ...]"""
        self._check(self.L.hmme_search_frame_bi_refs_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), d_other_mv,
                                                            d_other_ref, int(mv_per_ctu), d_center, d_pred, d_mv, d_sad, stream))

    def refine_frame_bi_refs_device(self, cur, refs, others, fp, d_other_mv, d_other_ref, mv_per_ctu, d_center, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost,
                                    stream=0):
        self._check(self.L.hmme_refine_frame_bi_refs_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), d_other_mv,
                                                            d_other_ref, int(mv_per_ctu), d_center, d_pred, d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def _frame_bi_refs(self, entry, cur, refs, others, sr, fen, other_mv, other_ref, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count, weights=None):
        """the *_frame_bi_refs and *_frame_bi_refs_w methods; int_mv: None for a search; weights: None or (searched list's, other list's) -> the
        two result tables [len(refs), count, 593, ...]"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        f, per = self._field(other_mv, n)
        rf = np.ascontiguousarray(other_ref, dtype=np.uint8).reshape(n, -1)
        assert rf.shape == (n, per)
        ptrs = []
        keep = []
        for a in (center_q, pred_q):
            if a is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.int16)
            assert a.shape == (len(refs), n, 2)
            keep.append(a)
            ptrs.append(a.ctypes.data)
        args = [f.ctypes.data, rf.ctypes.data, per] + ptrs
        if weights is not None:
            assert len(weights[0]) == len(refs) and len(weights[1]) == len(others)
            args = [self._weights(weights[0]), self._weights(weights[1])] + args
        if int_mv is not None:
            int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
            assert int_mv.shape == (len(refs), count, NUM_PARTS, 2)
            args += [int_mv.ctypes.data, int(use_hadamard)]
        mv = np.zeros((len(refs), count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((len(refs), count, NUM_PARTS), np.uint32)
        self._check(entry(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), *args, mv.ctypes.data, cost.ctypes.data))
        return mv, cost

    def search_frame_bi_refs(self, cur, refs, others, sr, other_mv, other_ref, center_q=None, pred_q=None, fen=1, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi_refs: host arrays -> (mv int16[n_refs,count,593,2], sad uint32[n_refs,count,593]).  other_mv: the other list's
        motion field (int16[n_ctu, 2] or [n_ctu, 1 | 64, 2]), other_ref: uint8[n_ctu] or [n_ctu, 1 | 64], the plane of `others` per block;
        center_q / pred_q: int16[n_refs, n_ctu, 2] or None"""
        return self._frame_bi_refs(self.L.hmme_search_frame_bi_refs, cur, refs, others, sr, fen, other_mv, other_ref, None, center_q, pred_q, True, ctu_first,
                                   ctu_count)

    def refine_frame_bi_refs(self, cur, refs, others, sr, other_mv, other_ref, int_mv, center_q=None, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi_refs: the refinement of integer winners int16[n_refs,count,593,2] against that origin -> (qmv, cost)"""
        return self._frame_bi_refs(self.L.hmme_refine_frame_bi_refs, cur, refs, others, sr, 1, other_mv, other_ref, int_mv, center_q, pred_q, use_hadamard,
                                   ctu_first, ctu_count)

    def select_dirs_refs_device(self, width, height, n_pics, n_refs_max, fp, sel, dirs, d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_uni_ref, d_pred,
                                d_field, d_ref, d_dir, d_slot=None, d_ctu_cost=None, stream=0):
        """hmme_select_dirs_refs_device: the refinement table sets of n_pics B pictures (device: uni and bi, each [n_pics, 2, n_refs_max, count, 593,
        ...]), the lists' uni fields int16[n_pics, 2, n_ctu, 64, 2] and reference indices uint8[n_pics, 2, n_ctu, 64] -> motion field and reference
        indices of those shapes, directions uint8[n_pics, n_ctu, 64], covering slots and CTU costs (d_slot / d_ctu_cost may be None).  dirs: one
        DirRefsParams per picture"""
        self._check(self.L.hmme_select_dirs_refs_device(self.h, int(width), int(height), int(n_pics), int(n_refs_max), C.byref(fp), C.byref(sel),
                                                        _dir_refs_params(dirs, n_pics), d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_uni_ref, d_pred,
                                                        d_field, d_ref, d_dir, d_slot, d_ctu_cost, stream))

    def select_dirs_refs_frame(self, width, height, sel, dir_params, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, pred_q=None, ctu_first=0, ctu_count=-1,
                               field=None, ref=None, dirs=None, slot=None, ctu_cost=None):
        """hmme_select_dirs_refs_frame: one picture, host arrays.  mv_uni / mv_bi int16[2, R, count, 593, 2], cost_uni / cost_bi uint32[2, R, count,
        593], uni_field int16[2, n_ctu, 64, 2], uni_ref uint8[2, n_ctu, 64], pred_q int16[2, R, n_ctu, 2] or None -> (field int16[2, n_ctu, 64, 2],
        ref uint8[2, n_ctu, 64], dirs uint8[n_ctu, 64], slot uint16[n_ctu, 64], ctu_cost uint32[n_ctu]); entries outside the CTU range keep the
        values of the arrays passed in (zeros when none is)"""
        R = int(np.shape(mv_uni)[1])
        call = lambda fp, *a: self.L.hmme_select_dirs_refs_frame(self.h, int(width), int(height), R, C.byref(fp), C.byref(sel), C.byref(dir_params), *a)
        return self._select_frame(call, (2, R), width, height, (mv_uni, cost_uni, mv_bi, cost_bi),
                                  ((uni_field, np.int16, (2,), (64, 2)), (uni_ref, np.uint8, (2,), (64,))), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (2,), (64, 2)), (ref, np.uint8, (2,), (64,)), (dirs, np.uint8, (), (64,)), (slot, np.uint16, (), (64,)),
                                   (ctu_cost, np.uint32, (), ())))

    def predict_bi_refs_device(self, refs0, refs1, fp, d_mv_field, d_dir_field, d_ref_field, mv_per_ctu, d_out, out_pitch_bytes, stream=0):
        """hmme_predict_bi_refs_device: the luma prediction of one B picture, every block from refs0[ref0] (L0), refs1[ref1] (L1) or both (averaged
        like TComYuv::addAvg): d_mv_field int16[2, n_ctu, mv_per_ctu, 2], d_dir_field uint8[n_ctu, mv_per_ctu], d_ref_field uint8[2, n_ctu,
        mv_per_ctu]; d_out = the device image"""
        self._check(self.L.hmme_predict_bi_refs_device(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), d_mv_field, d_dir_field,
                                                       d_ref_field, int(mv_per_ctu), d_out, int(out_pitch_bytes), stream))

    def predict_bi_refs_frame(self, refs0, refs1, mv_field, dir_field, ref_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi_refs_frame: the prediction of one B picture from list 0 (refs0) and list 1 (refs1) -> [height, width] array of the
        planes' sample type.  mv_field: int16[2, n_ctu, 2] or [2, n_ctu, 1 | 64, 2] quarter pels; dir_field: uint8[n_ctu] or [n_ctu, 1 | 64];
        ref_field: uint8[2, n_ctu] or [2, n_ctu, 1 | 64]; `out` keeps its samples outside the CTU range and in blocks without a direction or
        with an index >= the list's length"""
        r0 = refs0[0]
        f, per, df, fp = self._predict_fields(r0, r0.width, r0.height, mv_field, dir_field, 2, ctu_first, ctu_count)
        rf = np.ascontiguousarray(ref_field, dtype=np.uint8).reshape(2, df.shape[0], -1)
        assert rf.shape == (2,) + df.shape
        out = self._image(r0, out)
        self._check(self.L.hmme_predict_bi_refs_frame(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), f.ctypes.data, df.ctypes.data,
                                                      rf.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    # ---- the final prediction in a WP slice (include/hmme.h, "the final prediction in a slice with explicit weighted prediction"): weights
    # are (w0, offset, shift, round)
    def predict_bi_w_device(self, refs0, refs1, fp, weights0, weights1, d_mv_field, d_dir_field, mv_per_ctu, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_bi_w_device: predict_bi_device with two weights per picture (weights0[i] for refs0[i], weights1[i] for refs1[i]): uni
        blocks like predict_pairs_w_device, bi blocks like TComWeightPrediction::addWeightBi"""
        assert len(refs0) == len(refs1) == len(d_outs) == len(weights0) == len(weights1)
        oa = (C.c_void_p * len(d_outs))(*[int(o) for o in d_outs])
        self._check(self.L.hmme_predict_bi_w_device(self.h, _handles(refs0), _handles(refs1), len(refs0), C.byref(fp), self._weights(weights0),
                                                    self._weights(weights1), d_mv_field, d_dir_field, int(mv_per_ctu), oa, int(out_pitch_bytes), stream))

    def predict_bi_w_frame(self, ref0, ref1, wp0, wp1, mv_field, dir_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi_w_frame: predict_bi_frame with the weights wp0 (ref0) and wp1 (ref1)"""
        f, per, df, fp = self._predict_fields(ref0, ref0.width, ref0.height, mv_field, dir_field, 2, ctu_first, ctu_count)
        out = self._image(ref0, out)
        w0, w1 = (Weight(*[int(v) for v in w]) for w in (wp0, wp1))
        self._check(self.L.hmme_predict_bi_w_frame(self.h, ref0.h, ref1.h, C.byref(fp), C.byref(w0), C.byref(w1), f.ctypes.data, df.ctypes.data, per,
                                                   out.ctypes.data, out.shape[1]))
        return out

    def predict_refs_w_device(self, refs, fp, weights, d_mv_field, d_ref_field, mv_per_ctu, d_out, out_pitch_bytes, stream=0):
        """hmme_predict_refs_w_device: predict_refs_device with one weight per reference"""
        assert len(refs) == len(weights)
        self._check(self.L.hmme_predict_refs_w_device(self.h, _handles(refs), len(refs), C.byref(fp), self._weights(weights), d_mv_field, d_ref_field,
                                                      int(mv_per_ctu), d_out, int(out_pitch_bytes), stream))

    def predict_refs_w_frame(self, refs, weights, mv_field, ref_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_refs_w_frame: predict_refs_frame with one weight per reference"""
        assert len(refs) == len(weights)
        r0 = refs[0]
        f, per, rf, fp = self._predict_fields(r0, r0.width, r0.height, mv_field, ref_field, 1, ctu_first, ctu_count)
        out = self._image(r0, out)
        self._check(self.L.hmme_predict_refs_w_frame(self.h, _handles(refs), len(refs), C.byref(fp), self._weights(weights), f.ctypes.data, rf.ctypes.data, per,
                                                     out.ctypes.data, out.shape[1]))
        return out

    # ---- 4:2:0 chroma motion compensation from the luma motion fields (include/hmme.h, "4:2:0 chroma motion compensation"): planes, images and
    # weights come in component pairs (entry 2 i: Cb, 2 i + 1: Cr of picture / reference i); width, height: the LUMA size; weights None: none
    def _weights_or_none(self, weights, n):
        if weights is None:
            return None
        assert len(weights) == n
        return self._weights(weights)

    @staticmethod
    def _ptrs(addresses):
        return (C.c_void_p * len(addresses))(*[int(a) for a in addresses])

    def _chroma_images(self, plane, outs):
        """the (Cb, Cr) image pair of the predict_chroma_*_frame methods: `outs`, or zeros when None, each of the CHROMA plane's shape"""
        outs = (None, None) if outs is None else outs
        assert len(outs) == 2
        cb, cr = (self._image(plane, o) for o in outs)
        return cb, cr, self._ptrs([cb.ctypes.data, cr.ctypes.data])

    def predict_chroma_pairs_device(self, refs, width, height, fp, d_mv_field, mv_per_ctu, d_outs, out_pitch_bytes, weights=None, stream=0):
        """hmme_predict_chroma_pairs_device: the Cb and Cr prediction of up to 8 pictures from their LUMA motion fields; refs = [cb0, cr0, cb1, ...],
        d_outs = one device image address per plane, weights = one (w0, offset, shift, round) per plane or None"""
        assert len(refs) == len(d_outs) and len(refs) % 2 == 0
        self._check(self.L.hmme_predict_chroma_pairs_device(self.h, _handles(refs), len(refs) // 2, int(width), int(height), C.byref(fp),
                                                            self._weights_or_none(weights, len(refs)), d_mv_field, int(mv_per_ctu), self._ptrs(d_outs),
                                                            int(out_pitch_bytes), stream))

    def predict_chroma_frame(self, ref, width, height, mv_field, outs=None, weights=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_frame: ref = (cb, cr) planes of (width / 2) x (height / 2) -> (cb, cr) arrays [height / 2, width / 2] of the planes'
        sample type.  mv_field: the LUMA field, int16[n_ctu, 2] or [n_ctu, 1 | 64, 2] quarter pels; weights: None or one per component"""
        f, per, _, fp = self._predict_fields(ref[0], width, height, mv_field, None, 1, ctu_first, ctu_count)
        cb, cr, oa = self._chroma_images(ref[0], outs)
        self._check(self.L.hmme_predict_chroma_frame(self.h, _handles(ref), int(width), int(height), C.byref(fp), self._weights_or_none(weights, 2), f.ctypes.data,
                                                     per, oa, cb.shape[1]))
        return cb, cr

    def predict_chroma_refs_device(self, refs, width, height, fp, d_mv_field, d_ref_field, mv_per_ctu, d_out_cb, d_out_cr, out_pitch_bytes, weights=None, stream=0):
        """hmme_predict_chroma_refs_device: the Cb and Cr prediction of one picture, every block from the plane pair of refs = [cb0, cr0, cb1, ...]
        its reference index names (up to 8 references)"""
        assert len(refs) % 2 == 0
        self._check(self.L.hmme_predict_chroma_refs_device(self.h, _handles(refs), len(refs) // 2, int(width), int(height), C.byref(fp),
                                                           self._weights_or_none(weights, len(refs)), d_mv_field, d_ref_field, int(mv_per_ctu), d_out_cb, d_out_cr,
                                                           int(out_pitch_bytes), stream))

    def predict_chroma_refs_frame(self, refs, width, height, mv_field, ref_field, outs=None, weights=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_refs_frame: predict_refs_frame for Cb and Cr; refs = [cb0, cr0, cb1, cr1, ...] -> (cb, cr)"""
        assert len(refs) % 2 == 0
        f, per, rf, fp = self._predict_fields(refs[0], width, height, mv_field, ref_field, 1, ctu_first, ctu_count)
        cb, cr, oa = self._chroma_images(refs[0], outs)
        self._check(self.L.hmme_predict_chroma_refs_frame(self.h, _handles(refs), len(refs) // 2, int(width), int(height), C.byref(fp),
                                                          self._weights_or_none(weights, len(refs)), f.ctypes.data, rf.ctypes.data, per, oa, cb.shape[1]))
        return cb, cr

    # ---- prediction from one MV per 4x4 block (include/hmme.h, "prediction from one MV per 4x4 block"): the refs forms on the 256 layout --
    # what select_frame / select_refs_frame write with mv_per_ctu = 256; the reference field and the weights are optional
    def _field4(self, width, height, mv_field, ref_field):
        """host fields of the 256 layout: int16[n_ctu, 256, 2] and uint8[n_ctu, 256] or None -> (field, reference field or None, its address)"""
        n = self.L.hmme_num_ctus(int(width), int(height))
        f = np.ascontiguousarray(mv_field, dtype=np.int16)
        assert f.shape == (n, 256, 2)
        if ref_field is None:
            return f, None, None
        rf = np.ascontiguousarray(ref_field, dtype=np.uint8)
        assert rf.shape == (n, 256)
        return f, rf, rf.ctypes.data

    def predict_refs4_device(self, refs, fp, d_mv_field, d_ref_field, d_out, out_pitch_bytes, weights=None, stream=0):
        """hmme_predict_refs4_device: the luma prediction of one picture from d_mv_field int16[n_ctu, 256, 2] and d_ref_field uint8[n_ctu, 256]
        (None: every block from refs[0]); weights = one (w0, offset, shift, round) per reference or None; d_out = the device image"""
        self._check(self.L.hmme_predict_refs4_device(self.h, _handles(refs), len(refs), C.byref(fp), self._weights_or_none(weights, len(refs)), d_mv_field,
                                                     d_ref_field, d_out, int(out_pitch_bytes), stream))

    def predict_refs4_frame(self, refs, mv_field, ref_field=None, out=None, weights=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_refs4_frame: predict_refs_frame (with weights: predict_refs_w_frame) from one MV and one reference index per 4x4 block ->
        [height, width] array of the planes' sample type; `out` keeps its samples outside the CTU range and in blocks that are not live"""
        r0 = refs[0]
        f, rf, rf_ptr = self._field4(r0.width, r0.height, mv_field, ref_field)
        out = self._image(r0, out)
        fp = FrameParams(1, 0, r0.bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_refs4_frame(self.h, _handles(refs), len(refs), C.byref(fp), self._weights_or_none(weights, len(refs)), f.ctypes.data, rf_ptr,
                                                    out.ctypes.data, out.shape[1]))
        return out

    def predict_chroma_refs4_device(self, refs, width, height, fp, d_mv_field, d_ref_field, d_out_cb, d_out_cr, out_pitch_bytes, weights=None, stream=0):
        """hmme_predict_chroma_refs4_device: predict_chroma_refs_device from the fields of the 256 layout; refs = [cb0, cr0, cb1, ...], up to 8 references"""
        assert len(refs) % 2 == 0
        self._check(self.L.hmme_predict_chroma_refs4_device(self.h, _handles(refs), len(refs) // 2, int(width), int(height), C.byref(fp),
                                                            self._weights_or_none(weights, len(refs)), d_mv_field, d_ref_field, d_out_cb, d_out_cr, int(out_pitch_bytes),
                                                            stream))

    def predict_chroma_refs4_frame(self, refs, width, height, mv_field, ref_field=None, outs=None, weights=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_refs4_frame: predict_refs4_frame for Cb and Cr; refs = [cb0, cr0, cb1, cr1, ...] -> (cb, cr)"""
        assert len(refs) % 2 == 0
        f, rf, rf_ptr = self._field4(width, height, mv_field, ref_field)
        cb, cr, oa = self._chroma_images(refs[0], outs)
        fp = FrameParams(1, 0, refs[0].bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_chroma_refs4_frame(self.h, _handles(refs), len(refs) // 2, int(width), int(height), C.byref(fp),
                                                           self._weights_or_none(weights, len(refs)), f.ctypes.data, rf_ptr, oa, cb.shape[1]))
        return cb, cr

    def predict_chroma_bi_device(self, refs0, refs1, width, height, fp, d_mv_field, d_dir_field, mv_per_ctu, d_outs, out_pitch_bytes, weights0=None, weights1=None,
                                 stream=0):
        """hmme_predict_chroma_bi_device: the Cb and Cr prediction of up to 4 pictures whose blocks are L0, L1 or bi; refs0 / refs1 = [cb0, cr0, ...] of
        list 0 / list 1, fields as predict_bi_device takes them, d_outs = one device image address per plane of a list"""
        assert len(refs0) == len(refs1) == len(d_outs) and len(refs0) % 2 == 0
        self._check(self.L.hmme_predict_chroma_bi_device(self.h, _handles(refs0), _handles(refs1), len(refs0) // 2, int(width), int(height), C.byref(fp),
                                                         self._weights_or_none(weights0, len(refs0)), self._weights_or_none(weights1, len(refs1)), d_mv_field,
                                                         d_dir_field, int(mv_per_ctu), self._ptrs(d_outs), int(out_pitch_bytes), stream))

    def predict_chroma_bi_frame(self, ref0, ref1, width, height, mv_field, dir_field, outs=None, weights0=None, weights1=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_bi_frame: predict_bi_frame for Cb and Cr; ref0 / ref1 = (cb, cr) of list 0 / list 1 -> (cb, cr)"""
        f, per, df, fp = self._predict_fields(ref0[0], width, height, mv_field, dir_field, 2, ctu_first, ctu_count)
        cb, cr, oa = self._chroma_images(ref0[0], outs)
        self._check(self.L.hmme_predict_chroma_bi_frame(self.h, _handles(ref0), _handles(ref1), int(width), int(height), C.byref(fp),
                                                        self._weights_or_none(weights0, 2), self._weights_or_none(weights1, 2), f.ctypes.data, df.ctypes.data, per,
                                                        oa, cb.shape[1]))
        return cb, cr

    # ---- B pictures from one MV per 4x4 block (include/hmme.h, "B pictures from one MV per 4x4 block"): the bi pass, the decision and the
    # prediction on the 256 layout, one reference per list, unweighted
    def search_pairs_bi4_device(self, curs, refs, others, fp, d_other_mv, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_pairs_bi4_device: search_pairs_bi_device against origins built from d_other_mv int16[n_pairs, n_ctu, 256, 2]"""
        assert len(curs) == len(refs) == len(others)
        self._check(self.L.hmme_search_pairs_bi4_device(self.h, _handles(curs), _handles(refs), _handles(others), len(refs), C.byref(fp), d_other_mv, d_center, d_pred,
                                                        d_mv, d_sad, stream))

    def refine_pairs_bi4_device(self, curs, refs, others, fp, d_other_mv, d_center, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        """hmme_refine_pairs_bi4_device: refine_pairs_bi_device against origins built from d_other_mv int16[n_pairs, n_ctu, 256, 2]"""
        assert len(curs) == len(refs) == len(others)
        self._check(self.L.hmme_refine_pairs_bi4_device(self.h, _handles(curs), _handles(refs), _handles(others), len(refs), C.byref(fp), d_other_mv, d_center, d_pred,
                                                        d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def _frame_bi4(self, entry, cur, ref, other, sr, fen, other_mv, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count):
        """the two *_frame_bi4 methods (_frame_bi on the 256 layout); int_mv: None for a search -> the two result tables"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        f, _, _ = self._field4(cur.width, cur.height, other_mv, None)
        cq, cptr = self._pq(center_q, n)
        pq, pptr = self._pq(pred_q, n)
        args = [f.ctypes.data, cptr, pptr]
        if int_mv is not None:
            int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
            assert int_mv.shape == (count, NUM_PARTS, 2)
            args += [int_mv.ctypes.data, int(use_hadamard)]
        mv = np.zeros((count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((count, NUM_PARTS), np.uint32)
        self._check(entry(self.h, cur.h, ref.h, other.h, C.byref(fp), *args, mv.ctypes.data, cost.ctypes.data))
        return mv, cost

    def search_frame_bi4(self, cur, ref, other, sr, other_mv, center_q=None, pred_q=None, fen=1, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi4: search_frame_bi with other_mv int16[n_ctu, 256, 2], one MV per 4x4 block -> (mv int16[count,593,2], sad uint32[count,593])"""
        return self._frame_bi4(self.L.hmme_search_frame_bi4, cur, ref, other, sr, fen, other_mv, None, center_q, pred_q, True, ctu_first, ctu_count)

    def refine_frame_bi4(self, cur, ref, other, sr, other_mv, int_mv, center_q=None, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi4: refine_frame_bi with other_mv int16[n_ctu, 256, 2] -> (qmv int16[count,593,2], cost uint32[count,593])"""
        return self._frame_bi4(self.L.hmme_refine_frame_bi4, cur, ref, other, sr, 1, other_mv, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count)

    def select_dirs4_device(self, width, height, n_pics, fp, sel, dirs, d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_pred, d_field, d_dir,
                            d_slot=None, d_ctu_cost=None, stream=0):
        """hmme_select_dirs4_device: select_dirs_device over all 593 slots (sel.mv_per_ctu == 256; 8x4 / 4x8 PUs never bi): uni fields and motion
        field int16[n_pics, 2, n_ctu, 256, 2], directions uint8[n_pics, n_ctu, 256], covering slots uint16 of that shape"""
        self._check(self.L.hmme_select_dirs4_device(self.h, int(width), int(height), int(n_pics), C.byref(fp), C.byref(sel), _dir_params(dirs, n_pics),
                                                    d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_pred, d_field, d_dir, d_slot, d_ctu_cost, stream))

    def select_dirs4_frame(self, width, height, sel, dir_params, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, pred_q=None, ctu_first=0, ctu_count=-1,
                           field=None, dirs=None, slot=None, ctu_cost=None):
        """hmme_select_dirs4_frame: select_dirs_frame on the 256 layout: uni_field int16[2, n_ctu, 256, 2] -> (field int16[2, n_ctu, 256, 2], dirs
        uint8[n_ctu, 256], slot uint16[n_ctu, 256], ctu_cost uint32[n_ctu])"""
        call = lambda fp, *a: self.L.hmme_select_dirs4_frame(self.h, int(width), int(height), C.byref(fp), C.byref(sel), C.byref(dir_params), *a)
        return self._select_frame(call, (2,), width, height, (mv_uni, cost_uni, mv_bi, cost_bi), ((uni_field, np.int16, (2,), (256, 2)),), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (2,), (256, 2)), (dirs, np.uint8, (), (256,)), (slot, np.uint16, (), (256,)), (ctu_cost, np.uint32, (), ())))

    def _fields_bi4(self, width, height, mv_field, dir_field):
        """host fields of a B picture on the 256 layout: int16[2, n_ctu, 256, 2] and uint8[n_ctu, 256] -> contiguous arrays"""
        n = self.L.hmme_num_ctus(int(width), int(height))
        f = np.ascontiguousarray(mv_field, dtype=np.int16)
        df = np.ascontiguousarray(dir_field, dtype=np.uint8)
        assert f.shape == (2, n, 256, 2) and df.shape == (n, 256)
        return f, df

    def predict_bi4_device(self, refs0, refs1, fp, d_mv_field, d_dir_field, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_bi4_device: predict_bi_device from d_mv_field int16[n_pics, 2, n_ctu, 256, 2] and d_dir_field uint8[n_pics, n_ctu, 256]"""
        assert len(refs0) == len(refs1) == len(d_outs)
        self._check(self.L.hmme_predict_bi4_device(self.h, _handles(refs0), _handles(refs1), len(refs0), C.byref(fp), d_mv_field, d_dir_field, self._ptrs(d_outs),
                                                   int(out_pitch_bytes), stream))

    def predict_bi4_frame(self, ref0, ref1, mv_field, dir_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi4_frame: predict_bi_frame from one (direction, MV0, MV1) per 4x4 block: mv_field int16[2, n_ctu, 256, 2], dir_field
        uint8[n_ctu, 256] -> [height, width]; `out` keeps its samples outside the CTU range and in blocks without a direction"""
        f, df = self._fields_bi4(ref0.width, ref0.height, mv_field, dir_field)
        out = self._image(ref0, out)
        fp = FrameParams(1, 0, ref0.bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_bi4_frame(self.h, ref0.h, ref1.h, C.byref(fp), f.ctypes.data, df.ctypes.data, out.ctypes.data, out.shape[1]))
        return out

    def predict_chroma_bi4_device(self, refs0, refs1, width, height, fp, d_mv_field, d_dir_field, d_outs, out_pitch_bytes, stream=0):
        """hmme_predict_chroma_bi4_device: predict_chroma_bi_device (no weights) from the fields of the 256 layout; refs0 / refs1 = [cb0, cr0, ...]"""
        assert len(refs0) == len(refs1) == len(d_outs) and len(refs0) % 2 == 0
        self._check(self.L.hmme_predict_chroma_bi4_device(self.h, _handles(refs0), _handles(refs1), len(refs0) // 2, int(width), int(height), C.byref(fp), d_mv_field,
                                                          d_dir_field, self._ptrs(d_outs), int(out_pitch_bytes), stream))

    def predict_chroma_bi4_frame(self, ref0, ref1, width, height, mv_field, dir_field, outs=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_bi4_frame: predict_bi4_frame for Cb and Cr; ref0 / ref1 = (cb, cr) of list 0 / list 1 -> (cb, cr)"""
        f, df = self._fields_bi4(width, height, mv_field, dir_field)
        cb, cr, oa = self._chroma_images(ref0[0], outs)
        fp = FrameParams(1, 0, ref0[0].bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_chroma_bi4_frame(self.h, _handles(ref0), _handles(ref1), int(width), int(height), C.byref(fp), f.ctypes.data, df.ctypes.data,
                                                         oa, cb.shape[1]))
        return cb, cr

    # ---- B pictures with several references per list from one MV per 4x4 block (include/hmme.h, "B pictures with several references per
    # list from one MV per 4x4 block"): the bi_refs calls on the 256 layout, unweighted
    def search_frame_bi_refs4_device(self, cur, refs, others, fp, d_other_mv, d_other_ref, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_frame_bi_refs4_device: search_frame_bi_refs_device against the origin built from d_other_mv int16[n_ctu, 256, 2] and
        d_other_ref uint8[n_ctu, 256]: every 4x4 block from others[its index] (an index >= len(others) reads others[0])"""
        self._check(self.L.hmme_search_frame_bi_refs4_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), d_other_mv,
                                                             d_other_ref, d_center, d_pred, d_mv, d_sad, stream))

    def refine_frame_bi_refs4_device(self, cur, refs, others, fp, d_other_mv, d_other_ref, d_center, d_pred, d_int_mv, use_hadamard, d_qmv, d_cost, stream=0):
        """hmme_refine_frame_bi_refs4_device: refine_frame_bi_refs_device against that origin"""
        self._check(self.L.hmme_refine_frame_bi_refs4_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), d_other_mv,
                                                             d_other_ref, d_center, d_pred, d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def _frame_bi_refs4(self, entry, cur, refs, others, sr, fen, other_mv, other_ref, int_mv, center_q, pred_q, use_hadamard, ctu_first, ctu_count):
        """the two *_frame_bi_refs4 methods (_frame_bi_refs on the 256 layout); int_mv: None for a search -> the two result tables
        [len(refs), count, 593, ...]"""
        n = self.L.hmme_num_ctus(cur.width, cur.height)
        count = n - ctu_first if ctu_count < 0 else ctu_count
        fp = FrameParams(sr, int(fen), cur.bit_depth, ctu_first, count)
        f, rf, rf_ptr = self._field4(cur.width, cur.height, other_mv, other_ref)
        args = [f.ctypes.data, rf_ptr]
        keep = []
        for a in (center_q, pred_q):
            if a is None:
                args.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.int16)
            assert a.shape == (len(refs), n, 2)
            keep.append(a)
            args.append(a.ctypes.data)
        if int_mv is not None:
            int_mv = np.ascontiguousarray(int_mv, dtype=np.int16)
            assert int_mv.shape == (len(refs), count, NUM_PARTS, 2)
            args += [int_mv.ctypes.data, int(use_hadamard)]
        mv = np.zeros((len(refs), count, NUM_PARTS, 2), np.int16)
        cost = np.zeros((len(refs), count, NUM_PARTS), np.uint32)
        self._check(entry(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp), *args, mv.ctypes.data, cost.ctypes.data))
        return mv, cost

    def search_frame_bi_refs4(self, cur, refs, others, sr, other_mv, other_ref, center_q=None, pred_q=None, fen=1, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi_refs4: search_frame_bi_refs with other_mv int16[n_ctu, 256, 2] and other_ref uint8[n_ctu, 256], one entry per
        4x4 block (None: refused) -> (mv int16[n_refs,count,593,2], sad uint32[n_refs,count,593])"""
        return self._frame_bi_refs4(self.L.hmme_search_frame_bi_refs4, cur, refs, others, sr, fen, other_mv, other_ref, None, center_q, pred_q, True, ctu_first,
                                    ctu_count)

    def refine_frame_bi_refs4(self, cur, refs, others, sr, other_mv, other_ref, int_mv, center_q=None, pred_q=None, use_hadamard=True, ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi_refs4: refine_frame_bi_refs on the 256 layout -> (qmv int16[n_refs,count,593,2], cost uint32[n_refs,count,593])"""
        return self._frame_bi_refs4(self.L.hmme_refine_frame_bi_refs4, cur, refs, others, sr, 1, other_mv, other_ref, int_mv, center_q, pred_q, use_hadamard,
                                    ctu_first, ctu_count)

    def select_dirs_refs4_device(self, width, height, n_pics, n_refs_max, fp, sel, dirs, d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_uni_ref, d_pred,
                                 d_field, d_ref, d_dir, d_slot=None, d_ctu_cost=None, stream=0):
        """hmme_select_dirs_refs4_device: select_dirs_refs_device over all 593 slots (sel.mv_per_ctu == 256; 8x4 / 4x8 PUs never bi): uni fields and
        motion field int16[n_pics, 2, n_ctu, 256, 2], reference indices uint8[n_pics, 2, n_ctu, 256], directions uint8[n_pics, n_ctu, 256],
        covering slots uint16 of that shape"""
        self._check(self.L.hmme_select_dirs_refs4_device(self.h, int(width), int(height), int(n_pics), int(n_refs_max), C.byref(fp), C.byref(sel),
                                                         _dir_refs_params(dirs, n_pics), d_mv_uni, d_cost_uni, d_mv_bi, d_cost_bi, d_uni_field, d_uni_ref, d_pred,
                                                         d_field, d_ref, d_dir, d_slot, d_ctu_cost, stream))

    def select_dirs_refs4_frame(self, width, height, sel, dir_params, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, pred_q=None, ctu_first=0, ctu_count=-1,
                                field=None, ref=None, dirs=None, slot=None, ctu_cost=None):
        """hmme_select_dirs_refs4_frame: select_dirs_refs_frame on the 256 layout: uni_field int16[2, n_ctu, 256, 2], uni_ref uint8[2, n_ctu, 256] ->
        (field int16[2, n_ctu, 256, 2], ref uint8[2, n_ctu, 256], dirs uint8[n_ctu, 256], slot uint16[n_ctu, 256], ctu_cost uint32[n_ctu])"""
        R = int(np.shape(mv_uni)[1])
        call = lambda fp, *a: self.L.hmme_select_dirs_refs4_frame(self.h, int(width), int(height), R, C.byref(fp), C.byref(sel), C.byref(dir_params), *a)
        return self._select_frame(call, (2, R), width, height, (mv_uni, cost_uni, mv_bi, cost_bi),
                                  ((uni_field, np.int16, (2,), (256, 2)), (uni_ref, np.uint8, (2,), (256,))), pred_q, ctu_first, ctu_count,
                                  ((field, np.int16, (2,), (256, 2)), (ref, np.uint8, (2,), (256,)), (dirs, np.uint8, (), (256,)), (slot, np.uint16, (), (256,)),
                                   (ctu_cost, np.uint32, (), ())))

    def _fields_bi_refs4(self, width, height, mv_field, dir_field, ref_field):
        """host fields of a multi-reference B picture on the 256 layout: int16[2, n_ctu, 256, 2], uint8[n_ctu, 256], uint8[2, n_ctu, 256]"""
        f, df = self._fields_bi4(width, height, mv_field, dir_field)
        rf = np.ascontiguousarray(ref_field, dtype=np.uint8)
        assert rf.shape == (2,) + df.shape
        return f, df, rf

    def predict_bi_refs4_device(self, refs0, refs1, fp, d_mv_field, d_dir_field, d_ref_field, d_out, out_pitch_bytes, stream=0):
        """hmme_predict_bi_refs4_device: predict_bi_refs_device from d_mv_field int16[2, n_ctu, 256, 2], d_dir_field uint8[n_ctu, 256] and
        d_ref_field uint8[2, n_ctu, 256]; d_out = the device image"""
        self._check(self.L.hmme_predict_bi_refs4_device(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), d_mv_field, d_dir_field,
                                                        d_ref_field, d_out, int(out_pitch_bytes), stream))

    def predict_bi_refs4_frame(self, refs0, refs1, mv_field, dir_field, ref_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi_refs4_frame: predict_bi_refs_frame from one (direction, MV0, MV1, ref0, ref1) per 4x4 block -> [height, width]; `out`
        keeps its samples outside the CTU range and in blocks that are not live"""
        r0 = refs0[0]
        f, df, rf = self._fields_bi_refs4(r0.width, r0.height, mv_field, dir_field, ref_field)
        out = self._image(r0, out)
        fp = FrameParams(1, 0, r0.bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_bi_refs4_frame(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), f.ctypes.data, df.ctypes.data,
                                                       rf.ctypes.data, out.ctypes.data, out.shape[1]))
        return out

    def predict_chroma_bi_refs4_device(self, refs0, refs1, width, height, fp, d_mv_field, d_dir_field, d_ref_field, d_out_cb, d_out_cr, out_pitch_bytes, stream=0):
        """hmme_predict_chroma_bi_refs4_device: predict_chroma_bi_refs_device (no weights) from the fields of the 256 layout; refs0 / refs1 = [cb0,
        cr0, cb1, ...], up to 8 references in both lists together"""
        assert len(refs0) % 2 == 0 and len(refs1) % 2 == 0
        self._check(self.L.hmme_predict_chroma_bi_refs4_device(self.h, _handles(refs0), len(refs0) // 2, _handles(refs1), len(refs1) // 2, int(width), int(height),
                                                               C.byref(fp), d_mv_field, d_dir_field, d_ref_field, d_out_cb, d_out_cr, int(out_pitch_bytes), stream))

    def predict_chroma_bi_refs4_frame(self, refs0, refs1, width, height, mv_field, dir_field, ref_field, outs=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_chroma_bi_refs4_frame: predict_bi_refs4_frame for Cb and Cr; refs0 / refs1 = [cb0, cr0, cb1, cr1, ...] -> (cb, cr)"""
        assert len(refs0) % 2 == 0 and len(refs1) % 2 == 0
        f, df, rf = self._fields_bi_refs4(width, height, mv_field, dir_field, ref_field)
        cb, cr, oa = self._chroma_images(refs0[0], outs)
        fp = FrameParams(1, 0, refs0[0].bit_depth, ctu_first, ctu_count)
        self._check(self.L.hmme_predict_chroma_bi_refs4_frame(self.h, _handles(refs0), len(refs0) // 2, _handles(refs1), len(refs1) // 2, int(width), int(height),
                                                              C.byref(fp), f.ctypes.data, df.ctypes.data, rf.ctypes.data, oa, cb.shape[1]))
        return cb, cr

    # ---- multi-reference B pictures with explicit weights and in 4:2:0 (include/hmme.h, "multi-reference B pictures: explicit weights and
    # 4:2:0 chroma"): one (w0, offset, shift, round) per reference of each list; chroma: per plane, (Cb, Cr) per reference, or None
    def search_frame_bi_refs_w_device(self, cur, refs, others, fp, weights, other_weights, d_other_mv, d_other_ref, mv_per_ctu, d_center, d_pred, d_mv, d_sad, stream=0):
        """hmme_search_frame_bi_refs_w_device: search_frame_bi_refs_device in a WP slice: weights[r] prices the candidates of refs[r], other_weights[o]
        shapes the prediction of others[o] the ONE origin is built from"""
        assert len(refs) == len(weights) and len(others) == len(other_weights)
        self._check(self.L.hmme_search_frame_bi_refs_w_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp),
                                                              self._weights(weights), self._weights(other_weights), d_other_mv, d_other_ref, int(mv_per_ctu), d_center,
                                                              d_pred, d_mv, d_sad, stream))

    def refine_frame_bi_refs_w_device(self, cur, refs, others, fp, weights, other_weights, d_other_mv, d_other_ref, mv_per_ctu, d_center, d_pred, d_int_mv,
                                      use_hadamard, d_qmv, d_cost, stream=0):
        """hmme_refine_frame_bi_refs_w_device: refine_frame_bi_refs_device in a WP slice"""
        assert len(refs) == len(weights) and len(others) == len(other_weights)
        self._check(self.L.hmme_refine_frame_bi_refs_w_device(self.h, cur.h, _handles(refs), len(refs), _handles(others), len(others), C.byref(fp),
                                                              self._weights(weights), self._weights(other_weights), d_other_mv, d_other_ref, int(mv_per_ctu), d_center,
                                                              d_pred, d_int_mv, int(use_hadamard), d_qmv, d_cost, stream))

    def search_frame_bi_refs_w(self, cur, refs, others, sr, weights, other_weights, other_mv, other_ref, center_q=None, pred_q=None, ctu_first=0, ctu_count=-1):
        """hmme_search_frame_bi_refs_w: search_frame_bi_refs with one weight per reference of both lists (FEN is not consulted)"""
        return self._frame_bi_refs(self.L.hmme_search_frame_bi_refs_w, cur, refs, others, sr, 1, other_mv, other_ref, None, center_q, pred_q, True, ctu_first,
                                   ctu_count, weights=(weights, other_weights))

    def refine_frame_bi_refs_w(self, cur, refs, others, sr, weights, other_weights, other_mv, other_ref, int_mv, center_q=None, pred_q=None, use_hadamard=True,
                               ctu_first=0, ctu_count=-1):
        """hmme_refine_frame_bi_refs_w: refine_frame_bi_refs with one weight per reference of both lists"""
        return self._frame_bi_refs(self.L.hmme_refine_frame_bi_refs_w, cur, refs, others, sr, 1, other_mv, other_ref, int_mv, center_q, pred_q, use_hadamard,
                                   ctu_first, ctu_count, weights=(weights, other_weights))

    def predict_bi_refs_w_device(self, refs0, refs1, fp, weights0, weights1, d_mv_field, d_dir_field, d_ref_field, mv_per_ctu, d_out, out_pitch_bytes, stream=0):
        """hmme_predict_bi_refs_w_device: predict_bi_refs_device with weights0[r] for refs0[r] and weights1[r] for refs1[r]: uni blocks through
        addWeightUni with their reference's weight, bi blocks through addWeightBi with the two weights their indices name"""
        assert len(refs0) == len(weights0) and len(refs1) == len(weights1)
        self._check(self.L.hmme_predict_bi_refs_w_device(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), self._weights(weights0),
                                                         self._weights(weights1), d_mv_field, d_dir_field, d_ref_field, int(mv_per_ctu), d_out, int(out_pitch_bytes),
                                                         stream))

    def predict_bi_refs_w_frame(self, refs0, refs1, weights0, weights1, mv_field, dir_field, ref_field, out=None, ctu_first=0, ctu_count=-1):
        """hmme_predict_bi_refs_w_frame: predict_bi_refs_frame with one weight per reference of each list"""
        assert len(refs0) == len(weights0) and len(refs1) == len(weights1)
        r0 = refs0[0]
        f, per, df, fp = self._predict_fields(r0, r0.width, r0.height, mv_field, dir_field, 2, ctu_first, ctu_count)
        rf = np.ascontiguousarray(ref_field, dtype=np.uint8).reshape(2, df.shape[0], -1)
        assert rf.shape == (2,) + df.shape
        out = self._image(r0, out)
        self._check(self.L.hmme_predict_bi_refs_w_frame(self.h, _handles(refs0), len(refs0), _handles(refs1), len(refs1), C.byref(fp), self._weights(weights0),
                                                        self._weights(weights1), f.ctypes.data, df.ctypes.data, rf.ctypes.data, per, out.ctypes.data, out.shape[1]))
        return out

    def predict_chroma_bi_refs_device(self, refs0, refs1, width, height, fp, d_mv_field, d_dir_field, d_ref_field, mv_per_ctu, d_out_cb, d_out_cr, out_pitch_bytes,
                                      weights0=None, weights1=None, stream=0):
        """hmme_predict_chroma_bi_refs_device: the Cb and Cr prediction of one B picture, every block from the plane pairs of refs0 / refs1 = [cb0,
        cr0, cb1, ...] its two reference indices name (up to 8 references in both lists together); fields as predict_bi_refs_device takes them"""
        assert len(refs0) % 2 == 0 and len(refs1) % 2 == 0
        self._check(self.L.hmme_predict_chroma_bi_refs_device(self.h, _handles(refs0), len(refs0) // 2, _handles(refs1), len(refs1) // 2, int(width), int(height),
                                                              C.byref(fp), self._weights_or_none(weights0, len(refs0)), self._weights_or_none(weights1, len(refs1)),
                                                              d_mv_field, d_dir_field, d_ref_field, int(mv_per_ctu), d_out_cb, d_out_cr, int(out_pitch_bytes), stream))

    def predict_chroma_bi_refs_frame(self, refs0, refs1, width, height, mv_field, dir_field, ref_field, outs=None, weights0=None, weights1=None, ctu_first=0,
                                     ctu_count=-1):
        """hmme_predict_chroma_bi_refs_frame: predict_bi_refs_frame for Cb and Cr; refs0 / refs1 = [cb0, cr0, cb1, cr1, ...] -> (cb, cr)"""
        assert len(refs0) % 2 == 0 and len(refs1) % 2 == 0
        f, per, df, fp = self._predict_fields(refs0[0], width, height, mv_field, dir_field, 2, ctu_first, ctu_count)
        rf = np.ascontiguousarray(ref_field, dtype=np.uint8).reshape(2, df.shape[0], -1)
        assert rf.shape == (2,) + df.shape
        cb, cr, oa = self._chroma_images(refs0[0], outs)
        self._check(self.L.hmme_predict_chroma_bi_refs_frame(self.h, _handles(refs0), len(refs0) // 2, _handles(refs1), len(refs1) // 2, int(width), int(height),
                                                             C.byref(fp), self._weights_or_none(weights0, len(refs0)), self._weights_or_none(weights1, len(refs1)),
                                                             f.ctypes.data, df.ctypes.data, rf.ctypes.data, per, oa, cb.shape[1]))
        return cb, cr

    # ---- estimating explicit weighted-prediction parameters (include/hmme.h, "estimating explicit weighted-prediction parameters") ----
    def plane_stats(self, plane):
        """hmme_plane_stats: xCalcACDCParamSlice of one picture -> (dc_sum, ac) = (sum of the samples, sum of |sample - normDC|) over the picture
        area; kept in the plane until its next upload"""
        dc, ac = C.c_int64(), C.c_int64()
        self._check(self.L.hmme_plane_stats(plane.h, C.byref(dc), C.byref(ac)))
        return int(dc.value), int(ac.value)

    def wp_estimate(self, cur, refs, log2_denom_start=6):
        """hmme_wp_estimate: HM's luma weighted-prediction estimate for one current picture and the references of its slice (HM starts the
        denominator at 6, at 7 with more than three references) -> (weights, infos): one (w0, offset, shift, round) per reference, as the *_w
        calls take it, and one WpInfo each"""
        n = len(refs)
        ra = _handles(refs)
        wa, ia = (Weight * max(n, 1))(), (WpInfo * max(n, 1))()
        self._check(self.L.hmme_wp_estimate(self.h, cur.h, ra, n, int(log2_denom_start), wa, ia))
        return [(w.w0, w.offset, w.shift, w.round) for w in wa[:n]], list(ia[:n])

    def wp_estimate_420(self, cur3, refs3, log2_denom_start=6):
        """hmme_wp_estimate_420: HM's weighted-prediction estimate for a 4:2:0 slice, joint over the components; cur3 = (y, cb, cr) planes of the
        current picture, refs3 = one such triple per reference -> (luma_weights, chroma_weights, infos): one (w0, offset, shift, round) per
        reference, one (cb, cr) pair of them per reference -- flattened, what predict_chroma_* take as `weights` --, and 3 WpInfo per reference"""
        n = len(refs3)
        ca, ra = _handles(cur3), _handles([p for ref in refs3 for p in ref])
        wl, wc, ia = (Weight * max(n, 1))(), (Weight * max(2 * n, 1))(), (WpInfo * max(3 * n, 1))()
        self._check(self.L.hmme_wp_estimate_420(self.h, ca, ra, n, int(log2_denom_start), wl, wc, ia))
        unpack = lambda ws: [(w.w0, w.offset, w.shift, w.round) for w in ws]
        return unpack(wl[:n]), unpack(wc[:2 * n]), list(ia[:3 * n])

    def time_wp_estimate_passes(self, cur, refs, wp, stream=0, reps=5):
        """device time in ms of the estimator's passes on their own -> (the two statistics launches over `cur`, the SAD pass against `refs`)"""
        a, b = C.c_float(), C.c_float()
        ra = _handles(refs)
        w = Weight(*[int(v) for v in wp])
        self._check(self.L.hmme_test_time_wp_estimate_passes(self.h, cur.h, ra, len(refs), C.byref(w), stream, reps, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def time_bipred_origin(self, cur, other, d_other_mv, mv_per_ctu, stream=0, reps=5):
        """device time in ms of the origin pass of a bi-prediction search on its own (whole picture)"""
        ms = C.c_float()
        self._check(self.L.hmme_test_time_bipred_origin(self.h, cur.h, other.h, d_other_mv, int(mv_per_ctu), stream, reps, C.byref(ms)))
        return float(ms.value)

    def upload_status(self, stream=0):
        """waits for `stream`; raises if an asynchronous upload carried an out-of-range sample"""
        self._check(self.L.hmme_upload_status(self.h, stream))

    @property
    def call_block_address(self):
        """device address of the per-CTU call's current-block staging area (high-address test)"""
        return int(self.L.hmme_test_device_address(self.h, None))

    def search_frame_device(self, cur, ref, fp, d_pred, d_mv, d_sad, stream=0):
        self._check(self.L.hmme_search_frame_device(self.h, cur.h, ref.h, C.byref(fp), d_pred, d_mv, d_sad, stream))

    def time_search_kernel(self, cur, ref, fp, d_pred, d_mv, d_sad, stream=0, reps=3):
        ms = C.c_float()
        self._check(self.L.hmme_test_time_search_kernel(self.h, cur.h, ref.h, C.byref(fp), d_pred, d_mv, d_sad, stream, reps,
                                                   C.byref(ms)))
        return float(ms.value)


def build_id():
    """identifies the kernel sources + flags the loaded library was built from (hmme_build_id)"""
    return load().hmme_build_id().decode()


def weight_check(bit_depth, wp, refine=False):
    """hmme_weight_check: 0, or the HMME_ERR_* code with which a whole-picture call refuses the weight wp = (w0, offset, shift, round)
    at this bit depth (pure host arithmetic: needs no GPU)"""
    w = Weight(*[int(v) for v in wp])
    return int(load().hmme_weight_check(int(bit_depth), C.byref(w), 1 if refine else 0))


def bipred_check(bit_depth, refine=False):
    """hmme_bipred_check: 0, or the HMME_ERR_* code with which the whole-picture bi-prediction calls refuse this bit depth
    (pure host arithmetic: needs no GPU)"""
    return int(load().hmme_bipred_check(int(bit_depth), 1 if refine else 0))


def bipred_weight_check(bit_depth, wp, other_wp, refine=False):
    """hmme_bipred_weight_check: 0, or the HMME_ERR_* code with which the weighted whole-picture bi-prediction calls refuse the pair of weights
    (wp: the searched list's, other_wp: the other list's; None passes a null pointer) at this bit depth (pure host arithmetic: needs no GPU)"""
    w = None if wp is None else C.byref(Weight(*[int(v) for v in wp]))
    ow = None if other_wp is None else C.byref(Weight(*[int(v) for v in other_wp]))
    return int(load().hmme_bipred_weight_check(int(bit_depth), w, ow, 1 if refine else 0))


def predict_bi_weight_check(bit_depth, wp0, wp1):
    """hmme_predict_bi_weight_check: 0, or the HMME_ERR_* code with which hmme_predict_bi_w_device refuses a picture's two weights (wp0: list
    0's, wp1: list 1's; None passes a null pointer) at this bit depth (pure host arithmetic: needs no GPU)"""
    w0 = None if wp0 is None else C.byref(Weight(*[int(v) for v in wp0]))
    w1 = None if wp1 is None else C.byref(Weight(*[int(v) for v in wp1]))
    return int(load().hmme_predict_bi_weight_check(int(bit_depth), w0, w1))


def predict_bi_refs_weight_check(bit_depth, wps0, wps1, n0=None, n1=None):
    """hmme_predict_bi_refs_weight_check: 0, or the HMME_ERR_* code with which hmme_predict_bi_refs_w_device refuses the weights of a picture's two
    lists (wps0 / wps1: one (w0, offset, shift, round) per reference; None passes a null pointer; n0 / n1: the counts passed, default the
    lengths) at this bit depth (pure host arithmetic: needs no GPU)"""
    a0 = None if wps0 is None else Engine._weights(wps0)
    a1 = None if wps1 is None else Engine._weights(wps1)
    n0 = (0 if wps0 is None else len(wps0)) if n0 is None else n0
    n1 = (0 if wps1 is None else len(wps1)) if n1 is None else n1
    return int(load().hmme_predict_bi_refs_weight_check(int(bit_depth), a0, int(n0), a1, int(n1)))


def bipred_refs_weight_check(bit_depth, wps, other_wps, refine=False, n_refs=None, n_others=None):
    """hmme_bipred_refs_weight_check: 0, or the HMME_ERR_* code with which the *_frame_bi_refs_w calls refuse the weights of the searched list
    (wps) and of the other list (other_wps); None passes a null pointer; n_refs / n_others: the counts passed, default the lengths (pure host
    arithmetic: needs no GPU)"""
    a = None if wps is None else Engine._weights(wps)
    b = None if other_wps is None else Engine._weights(other_wps)
    n_refs = (0 if wps is None else len(wps)) if n_refs is None else n_refs
    n_others = (0 if other_wps is None else len(other_wps)) if n_others is None else n_others
    return int(load().hmme_bipred_refs_weight_check(int(bit_depth), a, int(n_refs), b, int(n_others), 1 if refine else 0))


def select_check(sel):
    """hmme_select_check: 0, or HMME_ERR_ARG when a field of the SelectParams lies outside its range (pure host arithmetic: needs no GPU)"""
    return int(load().hmme_select_check(C.byref(sel)))


def _handles(planes):
    """the handles of a list of planes as the array of pointers the C calls take"""
    return (C.c_void_p * len(planes))(*[p.h for p in planes])


def _ref_cost(ref_cost, n_refs):
    """n_refs host uint32 for the ref_cost argument of the hmme_select_refs_* calls (None: a null pointer = zeros)"""
    if ref_cost is None:
        return None
    assert len(ref_cost) == n_refs
    return (C.c_uint32 * max(n_refs, 1))(*[int(v) for v in ref_cost])


def ref_idx_bits(n_refs, ref_idx):
    """hmme_ref_idx_bits: HM's bits of reference index ref_idx in a list of n_refs (TEncSearch.cpp:3030-3037); -1 outside 0 <= ref_idx < n_refs <= 16"""
    return int(load().hmme_ref_idx_bits(int(n_refs), int(ref_idx)))


def select_refs_check(sel, n_pics, n_refs, ref_cost=None):
    """hmme_select_refs_check: 0, or HMME_ERR_ARG when the SelectParams, the number of pictures / references or a ref_cost lies outside its
    range (pure host arithmetic: needs no GPU).  ref_cost: a sequence of integers (any length: n_refs of them are read) or None"""
    rc = None if ref_cost is None else (C.c_uint32 * max(len(ref_cost), 16))(*[int(v) for v in ref_cost])   # at most 16 are ever read
    return int(load().hmme_select_refs_check(C.byref(sel), int(n_pics), int(n_refs), rc))


def _dir_params(dirs, n_pics):
    """n_pics DirParams as the array the hmme_select_dirs_* calls take"""
    assert len(dirs) == n_pics
    a = (DirParams * max(n_pics, 1))()
    for k, d in enumerate(dirs):
        a[k] = d
    return a


def select_dirs_check(sel, n_pics, dirs):
    """hmme_select_dirs_check: 0, or HMME_ERR_ARG when the SelectParams (mv_per_ctu 64, mv_unit 0, price_mv 0 only), the number of pictures
    (1..4) or a bit count (<= 4096) lies outside its range (pure host arithmetic: needs no GPU).  dirs: a sequence of DirParams (any length:
    n_pics of them are read) or None"""
    a = None
    if dirs is not None:
        a = (DirParams * max(len(dirs), 4))()
        for k, d in enumerate(dirs):
            a[k] = d
    return int(load().hmme_select_dirs_check(C.byref(sel), int(n_pics), a))


def select_dirs4_check(sel, n_pics, dirs):
    """hmme_select_dirs4_check: select_dirs_check for the 256 layout: mv_per_ctu 256, mv_unit 0, price_mv 0 only"""
    a = None
    if dirs is not None:
        a = (DirParams * max(len(dirs), 4))()
        for k, d in enumerate(dirs):
            a[k] = d
    return int(load().hmme_select_dirs4_check(C.byref(sel), int(n_pics), a))


def _dir_refs_params(dirs, n_pics):
    """n_pics DirRefsParams as the array the hmme_select_dirs_refs_* calls take"""
    assert len(dirs) == n_pics
    a = (DirRefsParams * max(n_pics, 1))()
    for k, d in enumerate(dirs):
        a[k] = d
    return a


def select_dirs_refs_check(sel, n_pics, n_refs_max, dirs):
    """hmme_select_dirs_refs_check: 0, or HMME_ERR_ARG for what select_dirs_check refuses, n_refs_max outside 1..8, an n_refs outside
    1..n_refs_max, a bit count above 4096 or l1_valid_mask bits at or above n_refs[1] (pure host arithmetic: needs no GPU).  dirs: a sequence
    of DirRefsParams (any length: n_pics of them are read) or None"""
    a = None
    if dirs is not None:
        a = (DirRefsParams * max(len(dirs), 4))()
        for k, d in enumerate(dirs):
            a[k] = d
    return int(load().hmme_select_dirs_refs_check(C.byref(sel), int(n_pics), int(n_refs_max), a))


def select_dirs_refs4_check(sel, n_pics, n_refs_max, dirs):
    """hmme_select_dirs_refs4_check: select_dirs_refs_check for the 256 layout: mv_per_ctu 256, mv_unit 0, price_mv 0 only"""
    a = None
    if dirs is not None:
        a = (DirRefsParams * max(len(dirs), 4))()
        for k, d in enumerate(dirs):
            a[k] = d
    return int(load().hmme_select_dirs_refs4_check(C.byref(sel), int(n_pics), int(n_refs_max), a))


def ocl_compat_params(lt_x, lt_y, sr):
    p = SearchParams()
    load().hmme_params_ocl_compat(C.byref(p), lt_x, lt_y, sr)
    return p


def set_search_range(pred_x_q, pred_y_q, sr, cu_x, cu_y, pic_w, pic_h):
    out = [C.c_int() for _ in range(4)]
    load().hmme_set_search_range(pred_x_q, pred_y_q, sr, cu_x, cu_y, pic_w, pic_h, *[C.byref(o) for o in out])
    return tuple(o.value for o in out)


def slot_index(part_size, depth, part_idx, abs_z_idx):
    return load().hmme_slot_index(part_size, depth, part_idx, abs_z_idx)


def slot_rect(slot):
    out = [C.c_int() for _ in range(4)]
    rc = load().hmme_slot_rect(slot, *[C.byref(o) for o in out])
    if rc != 0:
        raise HmmeError(f"slot {slot} out of range")
    return tuple(o.value for o in out)


def slot_key(slot):
    """hmme_slot_key, the inverse of slot_index -> (part_size, depth, part_idx, abs_z_idx)"""
    out = [C.c_int() for _ in range(4)]
    if load().hmme_slot_key(int(slot), *[C.byref(o) for o in out]) != 0:
        raise HmmeError(f"slot {slot} out of range")
    return tuple(o.value for o in out)
