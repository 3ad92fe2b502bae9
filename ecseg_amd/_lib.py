"""ctypes binding of libecseg_hip.so (include/ecseg_hip.h).  There is no CPU fallback: when the library is missing
or no MI355X is visible, every entry point raises."""
import contextlib
import ctypes as C
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# ECSEG_HIP_LIB: another build of the same library (A/B timing of two builds on one GPU box)
LIB_PATH = os.environ.get('ECSEG_HIP_LIB') or os.path.join(HERE, 'libecseg_hip.so')

EXPORTS = [
    'ecseg_abi_version', 'ecseg_create', 'ecseg_destroy', 'ecseg_last_error', 'ecseg_device_name', 'ecseg_stream',
    'ecseg_model_load', 'ecseg_model_flops_per_patch', 'ecseg_forward_patches', 'ecseg_forward_patches_f32', 'ecseg_read_tensor',
    'ecseg_segment_images', 'ecseg_segment_images_ex', 'ecseg_segment_images_dev', 'ecseg_set_images_per_group', 'ecseg_set_option', 'ecseg_preprocess', 'ecseg_u16_to_u8',
    'ecseg_meta_segment', 'ecseg_prefetch_input', 'ecseg_host_alloc', 'ecseg_host_free',
    'ecseg_stitch_argmax', 'ecseg_meta_inference', 'ecseg_meta_inference_dev', 'ecseg_count_cc', 'ecseg_ccl_labels',
    'ecseg_count_colocalization', 'ecseg_count_hsr', 'ecseg_overlay', 'ecseg_nuclei_regions', 'ecseg_nucleus_crops', 'ecseg_fish_distances', 'ecseg_fish_spots', 'ecseg_fish_render', 'ecseg_min_cut', 'ecseg_nuset_forward', 'ecseg_rpn_proposals', 'ecseg_rpn_proposals_last', 'ecseg_marker_watershed', 'ecseg_marker_watershed_batch', 'ecseg_marker_watershed_batch_bytes', 'ecseg_clean_nuclei', 'ecseg_rescale_down', 'ecseg_rescale_mask_up', 'ecseg_get_timings',
    'ecseg_set_kernel_profiling', 'ecseg_get_conv_profile', 'ecseg_get_conv_executed_flops', 'ecseg_get_conv_launch_profile', 'ecseg_debug_peek', 'ecseg_lzw_decode', 'ecseg_lzw_encode',
    'ecseg_comm_unique_id', 'ecseg_comm_create', 'ecseg_comm_destroy', 'ecseg_comm_last_error', 'ecseg_allgather_records', 'ecseg_allgather_records_dev',
    'ecseg_npy_write_i64', 'ecseg_png_write_labels', 'ecseg_png_write', 'ecseg_png_write_channel', 'ecseg_npy_label_info', 'ecseg_npy_read_labels_u8', 'ecseg_tiff_write_gray8', 'ecseg_tiff_info', 'ecseg_tiff_read',
    'ecseg_tiff_write_rgb8', 'ecseg_npy_write_i32_as_i64',
    'ecseg_tiff_encode_bound', 'ecseg_tiff_encode', 'ecseg_fish_render_tiff', 'ecseg_tiff_decode', 'ecseg_tiff_decode_routes',
    'ecseg_png_labels_encode', 'ecseg_meta_segment_files', 'ecseg_get_file_timings', 'ecseg_png_labels_stream_size',
    'ecseg_ccl_pass_debug', 'ecseg_meta_inference_stages_debug',
    'ecseg_tiff_decode_batch', 'ecseg_tiff_decode_batch_bytes', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_batch_counts',
    'ecseg_meta_segment_tiffs', 'ecseg_meta_segment_tiffs_files', 'ecseg_prefetch_tiffs', 'ecseg_get_read_timings',
    'ecseg_png_channel_bound', 'ecseg_png_channel_encode', 'ecseg_overlay_files',
    'ecseg_tiff_encode_batch', 'ecseg_tiff_encode_batch_bytes', 'ecseg_fish_render_tiff_batch',
    'ecseg_classify_nucleus_crops', 'ecseg_iseg_classifier_inputs_debug',
    'ecseg_marker_watershed_stages_debug', 'ecseg_marker_watershed_batch_stages_debug',
    'ecseg_interseg_batch',
    'ecseg_stitch_stages_debug', 'ecseg_preprocess_stages_debug', 'ecseg_otsu_debug',
    'ecseg_stat_fish_batch', 'ecseg_stat_fish_batch_bytes',
    'ecseg_min_cut_regions',
    'ecseg_scratch_fill_debug',
    'ecseg_fish_distances_batch',
]


class EcsegError(RuntimeError):
    """``code`` carries the ECSEG_E_* status of the failed call (None for binding-level errors)."""
    code = None


E_HIP = -2
E_NOMEM = -4
E_UNSUPPORTED, E_IO = -5, -6
ABI_VERSION = 6           # ECSEG_ABI_VERSION of include/ecseg_hip.h this binding was written for
TIFF_DEFLATE, TIFF_TILED, TIFF_PACKBITS = 1, 2, 4     # ECSEG_TIFF_* of the header: the kinds of file a TIFF decoder takes beside LZW and uncompressed strips
TIFF_OPTIONS = (('deflate', 'tiff_deflate_on_device', TIFF_DEFLATE), ('tiled', 'tiff_tiled_on_device', TIFF_TILED),
                ('packbits', 'tiff_packbits_on_device', TIFF_PACKBITS))   # (keyword, handle option and mirror attribute, bit)


def tiff_kinds(deflate=False, tiled=False, packbits=False):
    """The kinds word of the handle-free routing functions (ecseg_tiff_decode_routes and the three beside it) from three switches."""
    return (TIFF_DEFLATE if deflate else 0) | (TIFF_TILED if tiled else 0) | (TIFF_PACKBITS if packbits else 0)


def handle_tiff_kinds(handle):
    """The kinds word of anything that stands in for a ``Handle``: its ``tiff_kinds``, or the three mirror attributes where it has only those."""
    kinds = getattr(handle, 'tiff_kinds', None)
    return tiff_kinds(*(getattr(handle, key, False) for _, key, _ in TIFF_OPTIONS)) if kinds is None else int(kinds)


@contextlib.contextmanager
def tiff_options(handle, deflate=None, tiled=None, packbits=None):
    """The handle options ``tiff_deflate_on_device`` / ``tiff_tiled_on_device`` / ``tiff_packbits_on_device`` set to the given values
    for the body (None: left alone, and ``set_option`` is not needed).  An option that already stands as asked is not touched; each
    one that was changed is put back on the way out, also when the body raises.  ``Handle.tiff_options`` is this function."""
    changed = []
    try:
        for (_, key, _), value in zip(TIFF_OPTIONS, (deflate, tiled, packbits)):
            before = bool(getattr(handle, key, False))
            if value is not None and bool(value) != before:
                handle.set_option(key, int(bool(value)))
                changed.append((key, before))
        yield
    finally:
        for key, before in changed:
            handle.set_option(key, int(before))


class TensorDesc(C.Structure):
    _fields_ = [('buffer', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('c', C.c_int32),
                ('c_stride', C.c_int32), ('c_offset', C.c_int32)]


class OpDesc(C.Structure):
    _fields_ = [('op', C.c_int32), ('in0', C.c_int32), ('in1', C.c_int32), ('out', C.c_int32),
                ('kh', C.c_int32), ('kw', C.c_int32), ('stride', C.c_int32),
                ('pad_top', C.c_int32), ('pad_left', C.c_int32), ('act', C.c_int32), ('mode', C.c_int32),
                ('w0', C.c_int32), ('w1', C.c_int32), ('alpha', C.c_float), ('dilation', C.c_int32)]


class CclPassDesc(C.Structure):
    _fields_ = [('lut', C.c_uint32), ('conn', C.c_int32), ('stat', C.c_int32), ('aux_mode', C.c_int32), ('aux_c', C.c_int32),
                ('need', C.c_int32), ('count_only', C.c_int32), ('sparse', C.c_int32), ('allow_full', C.c_int32),
                ('n_queries', C.c_int32), ('query_key', C.c_int32 * 5), ('query_need', C.c_uint32 * 5)]


class CclPassOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ('root', 'area', 'sumy', 'sumx', 'flag', 'counters', 'list1', 'list2', 'tile_any')]


_lib = None


def rescale_extent(shape, scale):
    """The output extent of scikit-image's ``rescale``: ``np.round(scale * shape)``, half to even -> (out_h, out_w)."""
    out = np.round(scale * np.asarray(shape))
    return int(out[0]), int(out[1])


def rescale_weights(n_in, n_out):
    """The float64 weights ``rescale(anti_aliasing=True)`` filters one axis with (scipy 1.7's ``gaussian_filter1d``):
    sigma = max(0, (f - 1) / 2) with f = n_in / n_out, radius r = int(4 sigma + 0.5), exp(-0.5 / sigma^2 * x^2) over -r .. r divided by
    its sum; [1.0] (r = 0) where scipy copies the axis (sigma <= 1e-15)."""
    sigma = max(0.0, (float(np.float64(n_in) / np.float64(n_out)) - 1) / 2)
    if not sigma > 1e-15:
        return np.ones(1, np.float64)
    radius = int(4.0 * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return np.ascontiguousarray(phi / phi.sum(), np.float64)


def load_library():
    """Load libecseg_hip.so and declare the prototypes.  Raises EcsegError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EcsegError('%s not found: build it with `python -m ecseg_amd.build` (hipcc, gfx950)' % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise EcsegError('cannot load %s: %s' % (LIB_PATH, e))
    vp, i32, u8p = C.c_void_p, C.c_int, C.c_void_p
    lib.ecseg_abi_version.restype = C.c_int
    if lib.ecseg_abi_version() != ABI_VERSION:
        raise EcsegError('%s has ABI version %d, this binding was written for %d: rebuild it with `python -m ecseg_amd.build --force`'
                         % (LIB_PATH, lib.ecseg_abi_version(), ABI_VERSION))
    lib.ecseg_create.argtypes = [C.POINTER(vp), i32]
    lib.ecseg_destroy.argtypes = [vp]; lib.ecseg_destroy.restype = None
    lib.ecseg_last_error.argtypes = [vp]; lib.ecseg_last_error.restype = C.c_char_p
    lib.ecseg_device_name.argtypes = [vp, C.c_char_p, i32]
    lib.ecseg_stream.argtypes = [vp]; lib.ecseg_stream.restype = vp
    lib.ecseg_model_load.argtypes = [vp, C.POINTER(TensorDesc), i32, i32, C.POINTER(OpDesc), i32,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_int64), i32, i32, i32]
    lib.ecseg_model_flops_per_patch.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ecseg_forward_patches.argtypes = [vp, u8p, i32, vp]
    lib.ecseg_forward_patches_f32.argtypes = [vp, vp, i32, vp]
    lib.ecseg_read_tensor.argtypes = [vp, i32, i32, vp]
    lib.ecseg_segment_images.argtypes = [vp, u8p, i32, i32, i32, vp, vp, vp]
    lib.ecseg_segment_images_dev.argtypes = [vp, u8p, i32, i32, i32, vp, vp, vp]
    lib.ecseg_segment_images_ex.argtypes = [vp, u8p, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ecseg_set_images_per_group.argtypes = [vp, i32]
    lib.ecseg_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.ecseg_preprocess.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.ecseg_u16_to_u8.argtypes = [vp, vp, C.c_longlong, vp]
    lib.ecseg_meta_segment.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ecseg_prefetch_input.argtypes = [vp, vp, C.c_size_t]
    lib.ecseg_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.ecseg_host_free.argtypes = [vp, vp]
    lib.ecseg_stitch_argmax.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.ecseg_stitch_stages_debug.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.ecseg_preprocess_stages_debug.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ecseg_otsu_debug.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.ecseg_meta_inference.argtypes = [vp, u8p, i32, i32, i32, vp, vp]
    lib.ecseg_meta_inference_dev.argtypes = [vp, u8p, i32, i32, i32, vp, vp]
    lib.ecseg_meta_inference_stages_debug.argtypes = [vp, u8p, i32, i32, i32, i32, i32, vp, vp]
    lib.ecseg_count_cc.argtypes = [vp, u8p, i32, i32, i32, vp, vp]
    lib.ecseg_ccl_labels.argtypes = [vp, u8p, i32, i32, i32, i32, vp]
    lib.ecseg_ccl_pass_debug.argtypes = [vp, u8p, u8p, i32, i32, i32, C.POINTER(CclPassDesc), C.POINTER(CclPassOut)]
    lib.ecseg_scratch_fill_debug.argtypes = [vp, i32]
    lib.ecseg_count_colocalization.argtypes = [vp, u8p, u8p, i32, i32, i32, vp]
    lib.ecseg_count_hsr.argtypes = [vp, u8p, u8p, i32, i32, i32, i32, vp]
    lib.ecseg_overlay.argtypes = [vp, u8p, u8p, i32, i32, i32, i32, i32, i32, vp]
    lib.ecseg_nuclei_regions.argtypes = [vp, u8p, i32, i32, u8p, i32, i32, i32, i32, i32, vp, C.POINTER(C.c_int32)]
    lib.ecseg_nucleus_crops.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.ecseg_classify_nucleus_crops.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ecseg_iseg_classifier_inputs_debug.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.ecseg_interseg_batch.argtypes = [vp, vp, vp, vp, C.c_longlong, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecseg_fish_distances.argtypes = [vp, vp, i32, i32, u8p, i32, i32, i32, i32, vp, C.POINTER(C.c_int32)]
    lib.ecseg_fish_distances_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vp, i32, i32, i32, vp, vp, vp]
    lib.ecseg_fish_spots.argtypes = [vp, vp, i32, i32, u8p, i32, vp, i32, vp, i32, C.c_double, vp, i32, i32, i32, vp, vp, vp,
                                     C.POINTER(C.c_int32)]
    lib.ecseg_fish_render.argtypes = [vp, u8p, i32, i32, i32, vp, u8p, i32, u8p, vp, vp, vp]
    lib.ecseg_tiff_encode_bound.argtypes = [i32, i32, i32]; lib.ecseg_tiff_encode_bound.restype = C.c_longlong
    lib.ecseg_tiff_encode.argtypes = [vp, u8p, i32, i32, i32, i32, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    lib.ecseg_fish_render_tiff.argtypes = [vp, u8p, i32, i32, i32, vp, u8p, i32, u8p, C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong), vp, vp, vp]
    lib.ecseg_tiff_encode_batch.argtypes = [vp, vp, C.c_longlong, vp, i32, vp, C.c_longlong, vp]
    lib.ecseg_tiff_encode_batch_bytes.argtypes = [vp, i32]; lib.ecseg_tiff_encode_batch_bytes.restype = C.c_longlong
    lib.ecseg_fish_render_tiff_batch.argtypes = [vp, i32, C.POINTER(vp), vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp,
                                                 C.c_longlong, vp]
    lib.ecseg_stat_fish_batch.argtypes = [vp, i32, C.POINTER(vp), vp, vp, C.POINTER(vp), C.POINTER(vp), vp, C.POINTER(vp), vp, vp, vp, i32,
                                          C.POINTER(vp), C.POINTER(vp), i32, vp, vp, vp, vp, C.c_longlong, vp, vp, vp]
    lib.ecseg_stat_fish_batch_bytes.argtypes = [i32, vp, vp, vp, i32]; lib.ecseg_stat_fish_batch_bytes.restype = C.c_longlong
    lib.ecseg_tiff_decode.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.ecseg_tiff_decode_routes.argtypes = [vp, C.c_longlong, C.c_uint]
    lib.ecseg_tiff_decode_batch.argtypes = [vp, vp, C.c_longlong, vp, i32, vp, C.c_longlong, vp, vp, vp]
    lib.ecseg_tiff_decode_batch_bytes.argtypes = [vp, C.c_longlong, vp, i32, C.c_uint]; lib.ecseg_tiff_decode_batch_bytes.restype = C.c_longlong
    lib.ecseg_tiff_decode_batch_routes.argtypes = [vp, C.c_longlong, vp, i32, C.c_uint]
    lib.ecseg_tiff_decode_batch_counts.argtypes = [vp, C.c_longlong, C.c_uint]
    lib.ecseg_min_cut.argtypes = [vp, vp, C.c_longlong, vp, i32, i32, vp, vp]
    lib.ecseg_min_cut_regions.argtypes = [vp, vp, i32, i32, C.c_double, i32, i32, i32, C.c_longlong, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecseg_nuset_forward.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.ecseg_rpn_proposals.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, i32, i32, C.c_float, i32, i32, C.POINTER(C.c_int32), vp, vp, vp]
    lib.ecseg_rpn_proposals_last.argtypes = [vp, i32, vp, i32, i32, i32, C.c_float, i32, i32, C.POINTER(C.c_int32), vp, vp, vp]
    lib.ecseg_marker_watershed.argtypes = [vp, vp, i32, i32, vp, vp, vp, C.c_longlong, vp]
    lib.ecseg_marker_watershed_batch.argtypes = [vp, vp, C.c_longlong, vp, i32, vp, vp, vp, C.c_longlong, vp]
    lib.ecseg_marker_watershed_stages_debug.argtypes = [vp, vp, i32, i32, vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp]
    lib.ecseg_marker_watershed_batch_stages_debug.argtypes = [vp, vp, C.c_longlong, vp, i32, vp, vp, vp, C.c_longlong, vp, vp, vp, vp, vp]
    lib.ecseg_marker_watershed_batch_bytes.argtypes = [vp, i32, vp]; lib.ecseg_marker_watershed_batch_bytes.restype = C.c_longlong
    lib.ecseg_clean_nuclei.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.POINTER(C.c_double)]
    lib.ecseg_rescale_down.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp]
    lib.ecseg_rescale_mask_up.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.ecseg_get_timings.argtypes = [vp, vp]
    lib.ecseg_set_kernel_profiling.argtypes = [vp, i32]
    lib.ecseg_get_conv_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.ecseg_get_conv_executed_flops.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ecseg_debug_peek.argtypes = [vp, vp, i32]
    lib.ecseg_get_conv_launch_profile.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    for fn in (lib.ecseg_lzw_decode, lib.ecseg_lzw_encode):
        fn.argtypes = [vp, C.c_longlong, vp, C.c_longlong]
        fn.restype = C.c_longlong
    lib.ecseg_comm_unique_id.argtypes = [vp, i32]
    lib.ecseg_comm_create.argtypes = [C.POINTER(vp), vp, i32, i32, i32]
    lib.ecseg_comm_destroy.argtypes = [vp]; lib.ecseg_comm_destroy.restype = None
    lib.ecseg_comm_last_error.restype = C.c_char_p
    lib.ecseg_allgather_records.argtypes = [vp, vp, i32, vp]
    lib.ecseg_allgather_records_dev.argtypes = [vp, vp, i32, vp, vp]
    lib.ecseg_npy_write_i64.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ecseg_png_write_labels.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ecseg_png_labels_stream_size.argtypes = [vp, i32, i32, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.ecseg_png_labels_encode.argtypes = [vp, vp, i32, i32, i32, C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong)]
    lib.ecseg_meta_segment_files.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong),
                                             C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong), vp, vp, vp, vp]
    lib.ecseg_get_file_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.ecseg_png_channel_bound.argtypes = [i32, i32]; lib.ecseg_png_channel_bound.restype = C.c_longlong
    lib.ecseg_png_channel_encode.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong)]
    lib.ecseg_overlay_files.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, C.POINTER(vp), C.POINTER(vp), C.c_longlong,
                                        C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.ecseg_meta_segment_tiffs.argtypes = [vp, vp, C.c_longlong, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ecseg_meta_segment_tiffs_files.argtypes = [vp, vp, C.c_longlong, vp, i32, i32, i32, i32, i32, vp, C.POINTER(vp), C.c_longlong,
                                                   C.POINTER(C.c_longlong), C.POINTER(vp), C.c_longlong, C.POINTER(C.c_longlong), vp, vp, vp, vp]
    lib.ecseg_prefetch_tiffs.argtypes = [vp, vp, C.c_longlong, vp, i32, i32, i32, i32, i32]
    lib.ecseg_get_read_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.ecseg_png_write.argtypes = [C.c_char_p, vp, i32, i32, i32, i32]
    lib.ecseg_png_write_channel.argtypes = [C.c_char_p, vp, i32, i32, i32, i32, i32]
    lib.ecseg_npy_label_info.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]
    lib.ecseg_npy_read_labels_u8.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ecseg_tiff_write_gray8.argtypes = [C.c_char_p, vp, i32, i32, i32]
    lib.ecseg_tiff_write_rgb8.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ecseg_npy_write_i32_as_i64.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ecseg_tiff_info.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.ecseg_tiff_read.argtypes = [C.c_char_p, vp, C.c_longlong]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ('ecseg_abi_version',):
            fn.restype = C.c_int
    _lib = lib
    return lib


def pack_file_images(bufs):
    """1-D uint8 arrays -> (one buffer, (n, 2) int64 rows of byte offset and length): as ecseg_tiff_decode_batch takes its files.
    Views of one buffer in ascending order, clear of each other (how ``image_io.imread_many`` reads its files), are not copied."""
    sizes = np.array([b.size for b in bufs], np.int64)
    base = bufs[0].base if bufs else None
    if isinstance(base, np.ndarray) and base.dtype == np.uint8 and base.ndim == 1 and base.flags.c_contiguous and all(b.base is base for b in bufs):
        offs = np.array([b.ctypes.data - base.ctypes.data for b in bufs], np.int64)
        if (offs >= 0).all() and (offs + sizes <= base.size).all() and (offs[1:] >= (offs + sizes)[:-1]).all():
            return base, np.ascontiguousarray(np.stack([offs, sizes], axis=1))
    buf = np.concatenate(bufs) if bufs else np.zeros(0, np.uint8)
    return buf, np.ascontiguousarray(np.stack([np.cumsum(sizes) - sizes, sizes], axis=1))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8(a, shape_tail=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype != np.uint8:
        raise TypeError('expected a uint8 / bool array, got %s' % a.dtype)
    return a


def _file_u8(data):
    """the bytes of a file (``bytes``, ``bytearray``, ``memoryview`` or a uint8 array) -> a 1-D uint8 view of them"""
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else _u8(data).reshape(-1)
    if not buf.size:
        raise ValueError('tiff_decode takes the bytes of a file')
    return buf


class Handle:
    """One per GPU.  Owns the device context, its stream and all device buffers."""

    T_NAMES = ('tile', 'unet', 'tail', 'post', 'count')

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.ecseg_create(C.byref(h), int(device))
        if rc != 0:
            raise EcsegError('ecseg_create(device=%d) failed (%d): %s'
                             % (device, rc, self.lib.ecseg_last_error(None).decode()))
        self.h = h
        self.device = int(device)
        self.plan = None
        self.images_per_group = 0          # 0: automatic (ecseg_set_images_per_group)
        self.native_seconds = 0.0          # time spent inside ecseg_meta_segment (stage report of `make metaseg`)
        self._pinned = {}                  # page-locked host buffers of host_empty: array address -> allocation
        # mirrors of the three tiff_*_on_device options (set_option keeps them): what tiff_options restores from and tiff_kinds reads
        self.tiff_deflate_on_device = self.tiff_tiled_on_device = self.tiff_packbits_on_device = False

    def close(self):
        if getattr(self, 'h', None):
            for p in list(getattr(self, '_pinned', {}).values()):
                self.lib.ecseg_host_free(self.h, C.c_void_p(p))
            self._pinned = {}
            self.lib.ecseg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            e = EcsegError('%s failed (%d): %s' % (what, rc, self.lib.ecseg_last_error(self.h).decode()))
            e.code = rc
            raise e

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        self._check(self.lib.ecseg_device_name(self.h, buf, 256), 'ecseg_device_name')
        return buf.value.decode()

    @property
    def stream(self):
        return self.lib.ecseg_stream(self.h)

    # ---- model -----------------------------------------------------------------------------------
    def load_plan(self, plan):
        nt, no, nw = len(plan.tensors), len(plan.ops), len(plan.weights)
        T = (TensorDesc * nt)(*[TensorDesc(t['buffer'], t['h'], t['w'], t['c'], t['c_stride'], t['c_offset'])
                                for t in plan.tensors])
        O = (OpDesc * no)(*[OpDesc(o['op'], o['in0'], o['in1'], o['out'], o['kh'], o['kw'], o['stride'], o['pad_top'],
                                   o['pad_left'], o['act'], o['mode'], o['w0'], o['w1'], float(o['alpha']), int(o.get('dilation', 1)))
                            for o in plan.ops])
        keep = [np.ascontiguousarray(w, np.float32) for w in plan.weights]
        Wp = (C.c_void_p * max(nw, 1))(*[w.ctypes.data for w in keep])
        Wl = (C.c_int64 * max(nw, 1))(*[w.size for w in keep])
        self._check(self.lib.ecseg_model_load(self.h, T, nt, plan.n_buffers, O, no, Wp, Wl, nw, plan.input_tensor,
                                              plan.output_tensor), 'ecseg_model_load')
        self.plan = plan

    def flops_per_patch(self):
        v = C.c_double()
        self._check(self.lib.ecseg_model_flops_per_patch(self.h, C.byref(v)), 'ecseg_model_flops_per_patch')
        return v.value

    def set_images_per_group(self, n):
        self._check(self.lib.ecseg_set_images_per_group(self.h, int(n)), 'ecseg_set_images_per_group')
        self.images_per_group = int(n)

    def set_option(self, key, value):
        self._check(self.lib.ecseg_set_option(self.h, key.encode(), int(value)), 'ecseg_set_option(%s)' % key)
        if key in ('tiff_deflate_on_device', 'tiff_tiled_on_device', 'tiff_packbits_on_device'):
            setattr(self, key, bool(value))
        if key == 'images_per_group':        # the same knob as set_images_per_group: keep the mirror the OOM retry restores from
            self.images_per_group = int(value)

    def forward_patches(self, patches):
        """uint8 (or float32) (N, H, W, C) -> float32 (N, H', W', K): ``model.predict_on_batch`` (reference
        src/utils.py:115; the interSeg classifiers of src/interseg.py:155,168 return (N, K))."""
        if self.plan is None:
            raise EcsegError('no model loaded')
        p = np.ascontiguousarray(patches)
        is_f32 = p.dtype.kind == 'f'
        p = np.ascontiguousarray(p, np.float32) if is_f32 else _u8(p)
        ti, to = self.plan.tensors[self.plan.input_tensor], self.plan.tensors[self.plan.output_tensor]
        if p.ndim == 3:
            p = p[..., None]
        if p.shape[1:] != (ti['h'], ti['w'], ti['c']):
            raise ValueError('expected patches of shape (N, %d, %d, %d), got %s' % (ti['h'], ti['w'], ti['c'], p.shape))
        out = np.empty((p.shape[0], to['h'], to['w'], to['c']), np.float32)
        fn = self.lib.ecseg_forward_patches_f32 if is_f32 else self.lib.ecseg_forward_patches
        self._check(fn(self.h, _ptr(p), p.shape[0], _ptr(out)), 'ecseg_forward_patches')
        if getattr(self.plan, 'output_rank', 4) == 2:
            out = out.reshape(p.shape[0], to['c'])
        return out

    def read_tensor(self, tensor, n):
        t = self.plan.tensors[tensor]
        out = np.empty((n, t['h'], t['w'], t['c']), np.float32)
        self._check(self.lib.ecseg_read_tensor(self.h, int(tensor), int(n), _ptr(out)), 'ecseg_read_tensor')
        return out

    # ---- image pipeline -----------------------------------------------------------------------------
    def segment_images(self, gray, want_raw=True, want_tie_risk=False, want_probs=False):
        """(n, H, W) uint8 pre-processed images -> (raw labels | None, post-processed labels, n_ec)
        [+ tie_risk int32 (n,) when ``want_tie_risk``: pixels whose two largest uint8-quantised probabilities differ by at most
        1; + probs float32 (n, H, W, 4) when ``want_probs``: the stitched probabilities of src/utils.py:116]."""
        g = _u8(gray)
        if g.ndim == 2:
            g = g[None]
        n, H, W = g.shape
        raw = np.empty((n, H, W), np.uint8) if want_raw else None
        post = np.empty((n, H, W), np.uint8)
        nec = np.zeros(n, np.int32)
        if not (want_tie_risk or want_probs):
            self._check(self.lib.ecseg_segment_images(self.h, _ptr(g), n, H, W, _ptr(raw), _ptr(post), _ptr(nec)),
                        'ecseg_segment_images')
            return raw, post, nec
        tie = np.zeros(n, np.int32) if want_tie_risk else None
        probs = np.empty((n, H, W, 4), np.float32) if want_probs else None
        self._check(self.lib.ecseg_segment_images_ex(self.h, _ptr(g), n, H, W, _ptr(raw), _ptr(post), _ptr(nec), _ptr(tie), _ptr(probs)),
                    'ecseg_segment_images_ex')
        return (raw, post, nec) + ((tie,) if want_tie_risk else ()) + ((probs,) if want_probs else ())

    def segment_images_dev(self, gray_ptr, n, H, W, raw_ptr, post_ptr, nec_ptr):
        self._check(self.lib.ecseg_segment_images_dev(self.h, C.c_void_p(gray_ptr), n, H, W,
                                                      C.c_void_p(raw_ptr) if raw_ptr else None, C.c_void_p(post_ptr),
                                                      C.c_void_p(nec_ptr) if nec_ptr else None),
                    'ecseg_segment_images_dev')

    def preprocess(self, imgs):
        """(n, H, W[, C]) uint8 / uint16 -> ((n, H, W) uint8 gray, inverted flags): meta_preprocess."""
        a = np.ascontiguousarray(imgs)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError('meta_preprocess takes uint8 or uint16 images, got %s' % a.dtype)
        if a.ndim == 3:
            a = a[..., None]
        n, H, W, Cc = a.shape
        gray = np.empty((n, H, W), np.uint8)
        inv = np.zeros(n, np.int32)
        self._check(self.lib.ecseg_preprocess(self.h, _ptr(a), n, H, W, Cc, a.dtype.itemsize, _ptr(gray), _ptr(inv)),
                    'ecseg_preprocess')
        return gray, inv

    def meta_segment(self, imgs, gray_out=None, post_out=None):
        """(n, H, W[, C]) uint8 / uint16 raw images -> (gray, post-processed labels, n_ec, tie_risk): meta_preprocess + the
        segment pipeline in one device call (ecseg_meta_segment).  ``gray_out`` / ``post_out``: (n, H, W) uint8 arrays to
        fill (e.g. page-locked ones from ``host_empty``)."""
        a = np.ascontiguousarray(imgs)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError('meta_preprocess takes uint8 or uint16 images, got %s' % a.dtype)
        if a.ndim == 3:
            a = a[..., None]
        n, H, W, Cc = a.shape
        outs = []
        for o in (gray_out, post_out):
            if o is None:
                o = np.empty((n, H, W), np.uint8)
            elif o.shape != (n, H, W) or o.dtype != np.uint8 or not o.flags.c_contiguous:
                raise ValueError('output buffers must be C-contiguous uint8 arrays of shape %s' % ((n, H, W),))
            outs.append(o)
        nec = np.zeros(n, np.int32); tie = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        rc = self.lib.ecseg_meta_segment(self.h, _ptr(a), n, H, W, Cc, a.dtype.itemsize, _ptr(outs[0]), _ptr(outs[1]), _ptr(nec), _ptr(tie))
        self.native_seconds += time.perf_counter() - t0    # (inside the library, GIL released: `make metaseg`'s stage report)
        self._check(rc, 'ecseg_meta_segment')
        return outs[0], outs[1], nec, tie

    @staticmethod
    def _file_slots(buf, n, cap):
        """n slots of cap bytes in ``buf`` (a flat uint8 array, or None: a fresh one) -> the array and the table of their addresses"""
        if buf is None:
            buf = np.empty(n * cap, np.uint8)
        elif buf.dtype != np.uint8 or buf.ndim != 1 or buf.size < n * cap or not buf.flags.c_contiguous:
            raise ValueError('a file buffer must be a flat C-contiguous uint8 array of at least %d bytes' % (n * cap))
        return buf, (C.c_void_p * max(n, 1))(*[buf.ctypes.data + i * cap for i in range(n)])

    @staticmethod
    def _files_of(buf, sizes, cap, copy):
        """per slot the file (``bytes``, or with copy = False a view of the slot) or None for a file that did not fit"""
        out = []
        for i, k in enumerate(sizes):
            out.append(None if k <= 0 else buf[i * cap:i * cap + k].tobytes() if copy else buf[i * cap:i * cap + k])
        return out

    def png_labels_encode(self, labels, capacity=None):
        """(n, H, W) or (H, W) uint8 labels -> per image the bytes of the file ``image_io.write_label_png`` writes, run-length and
        Huffman coded on the device (ecseg_png_labels_encode); a list for a batch.  ``capacity``: bytes of each file's buffer, by
        default more than any label image needs; a file that does not fit is None, and ``last_file_bytes`` holds minus the size
        it needs (the lengths of the others)."""
        lab = np.ascontiguousarray(labels, np.uint8)
        single = lab.ndim == 2
        if single:
            lab = lab[None]
        if lab.ndim != 3 or lab.size == 0:
            raise ValueError('png_labels_encode takes non-empty (n, H, W) or (H, W) uint8 labels')
        n, H, W = lab.shape
        cap = 11 * H * W + 2 * H + 4096 if capacity is None else int(capacity)      # (a run costs at most 81 bits, a scan line 15 more)
        buf, ptrs = self._file_slots(None, n, max(cap, 1))
        sizes = (C.c_longlong * n)()
        self._check(self.lib.ecseg_png_labels_encode(self.h, _ptr(lab), n, H, W, ptrs, cap, sizes), 'ecseg_png_labels_encode')
        self.last_file_bytes = list(sizes)
        files = self._files_of(buf, self.last_file_bytes, max(cap, 1), True)
        return files[0] if single else files

    def png_channel_encode(self, pixels, channel, invert=False, capacity=None):
        """(n, H, W, C) or (H, W, C) uint8 pixels -> per image the bytes of the file ``image_io.write_png_channel(path, pixels_i, channel,
        invert)`` writes, coded on the device (ecseg_png_channel_encode); a list for a batch.  ``capacity``: bytes of each file's buffer,
        by default ecseg_png_channel_bound, which every file fits; a file that does not fit is None, and ``last_file_bytes`` holds
        minus the size it needs (the lengths of the others)."""
        a = np.ascontiguousarray(pixels, np.uint8)
        single = a.ndim == 3
        if single:
            a = a[None]
        if a.ndim != 4 or a.size == 0:
            raise ValueError('png_channel_encode takes non-empty (n, H, W, C) or (H, W, C) uint8 pixels')
        n, H, W, Cc = a.shape
        cap = int(self.lib.ecseg_png_channel_bound(H, W)) if capacity is None else int(capacity)
        buf, ptrs = self._file_slots(None, n, max(cap, 1))
        sizes = (C.c_longlong * n)()
        self._check(self.lib.ecseg_png_channel_encode(self.h, _ptr(a), n, H, W, Cc, int(channel), int(bool(invert)), ptrs, cap, sizes),
                    'ecseg_png_channel_encode')
        self.last_file_bytes = list(sizes)
        files = self._files_of(buf, self.last_file_bytes, max(cap, 1), True)
        return files[0] if single else files

    def overlay_files(self, labels, img, sensitivity, hsr_size_threshold=20):
        """``overlay(labels, u16_to_u8(img))`` and the red / green files of `make meta_overlay` from one upload (ecseg_overlay_files) ->
        (records, red_files, green_files): ``img`` is (n, H, W, C >= 2) uint8 or uint16 (or one image), the files are the bytes
        ``image_io.write_png_channel(path, I8_i, 0 / 1, invert=True)`` writes for the 8-bit image, which stays on the device.  Every
        file fits its buffer (ecseg_png_channel_bound), so none is None."""
        a, single = self._stack(labels)
        r = np.ascontiguousarray(img)
        if r.dtype not in (np.uint8, np.uint16):
            raise TypeError('overlay_files takes uint8 or uint16 images, got %s' % r.dtype)
        if r.ndim == 3:
            r = r[None]
        n, H, W = a.shape
        if r.ndim != 4 or r.shape[:3] != (n, H, W) or r.shape[3] < 2:
            raise ValueError('img must be (n, H, W, C>=2) matching labels')
        out = np.zeros((n, 12), np.int64)
        cap = int(self.lib.ecseg_png_channel_bound(H, W))
        rbuf, rptr = self._file_slots(None, n, cap)
        gbuf, gptr = self._file_slots(None, n, cap)
        rn, gn = (C.c_longlong * max(n, 1))(), (C.c_longlong * max(n, 1))()
        self._check(self.lib.ecseg_overlay_files(self.h, _ptr(a), _ptr(r), n, H, W, r.shape[3], r.dtype.itemsize, int(sensitivity),
                                                 int(hsr_size_threshold), _ptr(out), rptr, gptr, cap, rn, gn), 'ecseg_overlay_files')
        self.last_file_bytes = list(rn)[:n] + list(gn)[:n]
        red, green = self._files_of(rbuf, list(rn)[:n], cap, True), self._files_of(gbuf, list(gn)[:n], cap, True)
        return (out[0], red[0], green[0]) if single else (out, red, green)

    def meta_segment_files(self, imgs, gray_out=None, post_out=None, dapi_capacity=None, png_capacity=None, file_bufs=None):
        """``meta_segment`` plus, per image, the file images of ``dapi/<name>.tif`` (``write_tiff_gray8(gray, invert=True)``) and
        of ``labels/<stem>.png`` (``write_label_png(post)``), encoded on the device (ecseg_meta_segment_files) ->
        (gray, post, n_ec, tie_risk, dapi_files, png_files).  A file is ``bytes``, or None when it did not fit its capacity
        (defaults: H * W + 65536 and H * W // 2 + 65536 bytes; the caller then writes it from gray / post).  ``file_bufs``: two
        flat uint8 arrays of n * capacity bytes (e.g. page-locked ones) to build the files in; the files are then views of them."""
        a = np.ascontiguousarray(imgs)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError('meta_preprocess takes uint8 or uint16 images, got %s' % a.dtype)
        if a.ndim == 3:
            a = a[..., None]
        n, H, W, Cc = a.shape
        return self._segment_to_files('ecseg_meta_segment_files', (_ptr(a), n, H, W, Cc, a.dtype.itemsize), n, H, W, gray_out, post_out,
                                      dapi_capacity, png_capacity, file_bufs)

    def _segment_to_files(self, entry, head, n, H, W, gray_out, post_out, dapi_capacity, png_capacity, file_bufs):
        """what ``meta_segment_files`` and ``meta_segment_tiffs_files`` share: ``entry`` called with its own arguments (``head``, the
        input), then the file slots and the outputs -> (gray, post, n_ec, tie_risk, dapi_files, png_files)"""
        outs = self._gray_post(gray_out, post_out, n, H, W)
        dcap = H * W + 65536 if dapi_capacity is None else int(dapi_capacity)
        pcap = H * W // 2 + 65536 if png_capacity is None else int(png_capacity)
        dbuf, dptr = self._file_slots(file_bufs[0] if file_bufs else None, n, max(dcap, 1))
        pbuf, pptr = self._file_slots(file_bufs[1] if file_bufs else None, n, max(pcap, 1))
        dn, pn = (C.c_longlong * max(n, 1))(), (C.c_longlong * max(n, 1))()
        nec = np.zeros(n, np.int32); tie = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        rc = getattr(self.lib, entry)(self.h, *head, dptr, dcap, dn, pptr, pcap, pn, _ptr(outs[0]), _ptr(outs[1]), _ptr(nec), _ptr(tie))
        self.native_seconds += time.perf_counter() - t0
        self._check(rc, entry)
        self.last_file_bytes = list(dn)[:n] + list(pn)[:n]
        copy = not file_bufs
        return (outs[0], outs[1], nec, tie, self._files_of(dbuf, list(dn)[:n], max(dcap, 1), copy), self._files_of(pbuf, list(pn)[:n], max(pcap, 1), copy))

    def file_timings(self):
        """Device milliseconds of the last ``meta_segment_files`` call's dapi encode and PNG kernels."""
        ms = (C.c_float * 2)()
        self._check(self.lib.ecseg_get_file_timings(self.h, ms), 'ecseg_get_file_timings')
        return {'dapi': float(ms[0]), 'png': float(ms[1])}

    @staticmethod
    def _tiffs_packed(datas, shape):
        """the files of one ``meta_segment_tiffs`` call -> (buffer, ranges, n, H, W, C, bytes per sample); ``shape``: the batch's common
        (H, W, samples per pixel, bits per sample), a row of ``tiff_decode_packed``'s shapes"""
        bufs = [_file_u8(d) for d in datas]
        buf, ranges = pack_file_images(bufs)
        H, W, Cc, bits = (int(v) for v in shape)
        if bits not in (8, 16):
            raise ValueError('meta_segment_tiffs takes 8- or 16-bit samples, got %d bits' % bits)
        return buf, ranges, len(bufs), H, W, Cc, bits // 8

    def meta_segment_tiffs(self, datas, shape, gray_out=None, post_out=None):
        """``meta_segment`` on the bytes of n TIFF files of one ``shape`` (H, W, samples per pixel, bits per sample), decoded on the
        device straight into the batch (ecseg_meta_segment_tiffs) -> (gray, post, n_ec, tie_risk, status).  status[i] is 0, or the
        code ``tiff_decode`` fails with for file i alone (a file of another shape: -1); such an image is the all-zero image and its
        n_ec is -1.  Files that are views of one buffer in ascending order (``pack_file_images``) are not copied: with
        ``prefetch_tiffs`` that buffer is page-locked."""
        buf, ranges, n, H, W, Cc, bps = self._tiffs_packed(datas, shape)
        outs = self._gray_post(gray_out, post_out, n, H, W)
        nec = np.zeros(n, np.int32); tie = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        rc = self.lib.ecseg_meta_segment_tiffs(self.h, _ptr(buf), buf.size, _ptr(ranges), n, H, W, Cc, bps, _ptr(status), _ptr(outs[0]), _ptr(outs[1]),
                                               _ptr(nec), _ptr(tie))
        self.native_seconds += time.perf_counter() - t0
        self._check(rc, 'ecseg_meta_segment_tiffs')
        return outs[0], outs[1], nec, tie, status.tolist()

    def meta_segment_tiffs_files(self, datas, shape, gray_out=None, post_out=None, dapi_capacity=None, png_capacity=None, file_bufs=None):
        """``meta_segment_files`` on the bytes of n TIFF files (ecseg_meta_segment_tiffs_files) -> (gray, post, n_ec, tie_risk, dapi_files,
        png_files, status); the arguments behind ``shape`` and the files are ``meta_segment_files``'s, status is ``meta_segment_tiffs``'s.
        An image whose status is not 0 has no files (None)."""
        buf, ranges, n, H, W, Cc, bps = self._tiffs_packed(datas, shape)
        status = np.zeros(n, np.int32)
        return self._segment_to_files('ecseg_meta_segment_tiffs_files', (_ptr(buf), buf.size, _ptr(ranges), n, H, W, Cc, bps, _ptr(status)), n, H, W,
                                      gray_out, post_out, dapi_capacity, png_capacity, file_bufs) + (status.tolist(),)

    @staticmethod
    def _gray_post(gray_out, post_out, n, H, W):
        outs = []
        for o in (gray_out, post_out):
            if o is None:
                o = np.empty((n, H, W), np.uint8)
            elif o.shape != (n, H, W) or o.dtype != np.uint8 or not o.flags.c_contiguous:
                raise ValueError('output buffers must be C-contiguous uint8 arrays of shape %s' % ((n, H, W),))
            outs.append(o)
        return outs

    def prefetch_tiffs(self, datas, shape=None):
        """Name the files of the ``meta_segment_tiffs[_files]`` call AFTER the coming one, as that call will pass them (views of one
        page-locked buffer, unchanged until then): the coming call uploads and decodes them under its kernels
        (ecseg_prefetch_tiffs).  None withdraws."""
        if datas is None:
            self._check(self.lib.ecseg_prefetch_tiffs(self.h, None, 0, None, 0, 0, 0, 0, 0), 'ecseg_prefetch_tiffs')
            return
        buf, ranges, n, H, W, Cc, bps = self._tiffs_packed(datas, shape)
        self._check(self.lib.ecseg_prefetch_tiffs(self.h, _ptr(buf), buf.size, _ptr(ranges), n, H, W, Cc, bps), 'ecseg_prefetch_tiffs')

    def read_timings(self):
        """Device milliseconds of the TIFF decode kernels that served the last ``meta_segment_tiffs[_files]`` call."""
        ms = (C.c_float * 1)()
        self._check(self.lib.ecseg_get_read_timings(self.h, ms), 'ecseg_get_read_timings')
        return {'decode': float(ms[0])}

    def prefetch_input(self, imgs):
        """Name the raw images (a C-contiguous array in page-locked memory) of the meta_segment call AFTER the coming one: the
        coming call uploads them under its kernels (ecseg_prefetch_input).  None withdraws."""
        if imgs is None:
            self._check(self.lib.ecseg_prefetch_input(self.h, None, 0), 'ecseg_prefetch_input')
            return
        if not imgs.flags.c_contiguous:
            raise ValueError('prefetch_input takes a C-contiguous array')
        self._check(self.lib.ecseg_prefetch_input(self.h, _ptr(imgs), imgs.nbytes), 'ecseg_prefetch_input')

    def host_empty(self, shape, dtype=np.uint8):
        """An uninitialised numpy array in page-locked host memory (ecseg_host_alloc).  The memory belongs to the handle: it is
        released by ``host_release(array)`` or when the handle closes, and must not be used after that."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        p = C.c_void_p()
        rc = self.lib.ecseg_host_alloc(self.h, max(nbytes, 1), C.byref(p))     # (thread-safe: does not touch the handle's error text)
        if rc != 0:
            e = EcsegError('ecseg_host_alloc(%d bytes) failed (%d)' % (nbytes, rc))
            e.code = rc
            raise e
        arr = np.ctypeslib.as_array((C.c_uint8 * max(nbytes, 1)).from_address(p.value))[:nbytes].view(dtype).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_release(self, arr):
        p = self._pinned.pop(arr.ctypes.data, None)
        if p is not None and self.h:
            rc = self.lib.ecseg_host_free(self.h, C.c_void_p(p))
            if rc != 0:
                e = EcsegError('ecseg_host_free failed (%d)' % rc)
                e.code = rc
                raise e

    def u16_to_u8(self, a):
        a = np.ascontiguousarray(a, np.uint16)
        out = np.empty(a.shape, np.uint8)
        self._check(self.lib.ecseg_u16_to_u8(self.h, _ptr(a), a.size, _ptr(out)), 'ecseg_u16_to_u8')
        return out

    def stitch_argmax(self, probs, n_img, H, W):
        p = np.ascontiguousarray(probs, np.float32)
        out = np.empty((n_img, H, W), np.uint8)
        self._check(self.lib.ecseg_stitch_argmax(self.h, _ptr(p), n_img, H, W, _ptr(out)), 'ecseg_stitch_argmax')
        return out

    def stitch_stages(self, probs, n_img, H, W):
        """Test-only (ecseg_stitch_stages_debug): (n_img * n_patches, 256, 256, cs >= 4) float32 patch predictions, the whole batch in
        one launch -> dict: ``labels`` (n_img, H, W) uint8, ``tie_risk`` (n_img) int32, ``probs`` (n_img, H, W, 4) float32."""
        p = np.ascontiguousarray(probs, np.float32)
        if p.ndim != 4 or p.shape[1:3] != (256, 256) or (n_img and p.shape[0] % n_img):
            raise ValueError('probs must be (n_img * n_patches, 256, 256, channels), got %s' % (p.shape,))
        res = dict(labels=np.empty((n_img, H, W), np.uint8), tie_risk=np.empty(n_img, np.int32), probs=np.empty((n_img, H, W, 4), np.float32))
        self._check(self.lib.ecseg_stitch_stages_debug(self.h, _ptr(p), p.shape[3], n_img, H, W, _ptr(res['labels']), _ptr(res['tie_risk']),
                                                       _ptr(res['probs'])), 'ecseg_stitch_stages_debug')
        return res

    def preprocess_stages(self, imgs):
        """Test-only (ecseg_preprocess_stages_debug): ``preprocess`` with what it leaves on the way -> dict: ``hist`` (n, 256) uint32,
        ``threshold`` (n) int32, ``inverted`` (n) int32, ``gray`` (n, H, W) uint8."""
        a = np.ascontiguousarray(imgs)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError('meta_preprocess takes uint8 or uint16 images, got %s' % a.dtype)
        if a.ndim == 3:
            a = a[..., None]
        n, H, W, Cc = a.shape
        res = dict(hist=np.empty((n, 256), np.uint32), threshold=np.empty(n, np.int32), inverted=np.empty(n, np.int32),
                   gray=np.empty((n, H, W), np.uint8))
        self._check(self.lib.ecseg_preprocess_stages_debug(self.h, _ptr(a), n, H, W, Cc, a.dtype.itemsize, _ptr(res['hist']),
                                                           _ptr(res['threshold']), _ptr(res['inverted']), _ptr(res['gray'])),
                    'ecseg_preprocess_stages_debug')
        return res

    def otsu(self, hists, px):
        """Test-only (ecseg_otsu_debug): (n, 256) histograms with their pixel counts (n), each the sum of its histogram ->
        (threshold (n) int32, inverted (n) int32) of the Otsu kernel alone."""
        hs = np.ascontiguousarray(hists, np.uint32)
        p = np.ascontiguousarray(px, np.int64)
        if hs.ndim != 2 or hs.shape[1] != 256 or p.shape != (hs.shape[0],):
            raise ValueError('hists must be (n, 256) and px (n), got %s and %s' % (hs.shape, p.shape))
        thr, inv = np.empty(len(hs), np.int32), np.empty(len(hs), np.int32)
        self._check(self.lib.ecseg_otsu_debug(self.h, _ptr(hs), len(hs), _ptr(p), _ptr(thr), _ptr(inv)), 'ecseg_otsu_debug')
        return thr, inv

    def meta_inference(self, labels):
        a = _u8(labels)
        single = a.ndim == 2
        if single:
            a = a[None]
        n, H, W = a.shape
        out = np.empty_like(a)
        nec = np.zeros(n, np.int32)
        self._check(self.lib.ecseg_meta_inference(self.h, _ptr(a), n, H, W, _ptr(out), _ptr(nec)), 'ecseg_meta_inference')
        return (out[0], int(nec[0])) if single else (out, nec)

    def meta_inference_dev(self, in_ptr, n, H, W, out_ptr, nec_ptr):
        self._check(self.lib.ecseg_meta_inference_dev(self.h, C.c_void_p(in_ptr), n, H, W, C.c_void_p(out_ptr),
                                                      C.c_void_p(nec_ptr) if nec_ptr else None), 'ecseg_meta_inference_dev')

    def meta_inference_stages(self, labels, first, last, want_kill=False):
        """Test-only (ecseg_meta_inference_stages_debug): stages ``first`` .. ``last`` of meta_inference alone on (n, H, W) or
        (H, W) uint8 labels, the input of stage ``first`` -> the image after stage ``last`` (1 fill_holes(1), 2 fill_holes(2),
        3 size_thresh + ec_band_removal, 4 nucleus_in_metaphase, 5 merge_comp(1), 6 merge_comp(2) + the final dilation).
        ``want_kill``: -> (image, kill), kill = 1 at the pixels of the nuclei stage 4 erases (zeros when the range has no stage 4)."""
        a = _u8(labels)
        single = a.ndim == 2
        if single:
            a = a[None]
        n, H, W = a.shape
        out = np.empty_like(a)
        kill = np.zeros_like(a) if want_kill else None
        self._check(self.lib.ecseg_meta_inference_stages_debug(self.h, _ptr(a), n, H, W, int(first), int(last), _ptr(out), _ptr(kill)),
                    'ecseg_meta_inference_stages_debug')
        if single:
            out, kill = out[0], (kill[0] if want_kill else None)
        return (out, kill) if want_kill else out

    # ---- counting -----------------------------------------------------------------------------------
    @staticmethod
    def _stack(a):
        a = _u8(a)
        return (a[None], True) if a.ndim == 2 else (a, False)

    def count_cc(self, mask):
        a, single = self._stack(mask)
        n, H, W = a.shape
        cnt = np.zeros(n, np.int32); px = np.zeros(n, np.int64)
        self._check(self.lib.ecseg_count_cc(self.h, _ptr(a), n, H, W, _ptr(cnt), _ptr(px)), 'ecseg_count_cc')
        return (int(cnt[0]), int(px[0])) if single else (cnt, px)

    def ccl_labels(self, mask, connectivity=8):
        a, single = self._stack(mask)
        n, H, W = a.shape
        out = np.empty((n, H, W), np.int32)
        self._check(self.lib.ecseg_ccl_labels(self.h, _ptr(a), n, H, W, int(connectivity), _ptr(out)), 'ecseg_ccl_labels')
        return out[0] if single else out

    def ccl_pass(self, key, aux=None, lut=0xffffffff, conn=8, stat=0, aux_mode=0, aux_c=0, need=0, count_only=False, sparse=False,
                 allow_full=False, queries=()):
        """Test-only (ecseg_ccl_pass_debug): ONE labelling pass on (n, H, W) uint8 keys, described as the drivers of
        csrc/meta_inference_kernels.hip and csrc/overlay_kernels.hip describe theirs, with everything it produced -> dict: ``root`` int32 (-1 unkeyed, else the pixel
        index of the component's first pixel; after a count_only pass the pixel's own index where it was counted as a root),
        ``area`` uint32 / ``sumy`` / ``sumx`` uint64 / ``flag`` uint32 at root pixels (0 elsewhere), ``ncomp`` / ``npx`` (n, 3) for
        keys 1..3, ``last_root`` (last root + 1), ``cnt`` (n, 5) answers to ``queries`` [(key, need_bits)], ``list1`` / ``list2``
        (per image the roots of value 1 / 2, in the device's order) and ``tile_any`` (n, ceil(H/32), ceil(W/64))."""
        a, _ = self._stack(key)
        n, H, W = a.shape
        x = None
        if aux is not None:
            x, _ = self._stack(aux)
            if x.shape != a.shape:
                raise ValueError('aux must have the shape of key')
        queries = list(queries)
        if len(queries) > 5:
            raise ValueError('at most 5 flag queries')
        d = CclPassDesc(lut=int(lut), conn=int(conn), stat=int(stat), aux_mode=int(aux_mode), aux_c=int(aux_c), need=int(need),
                        count_only=int(bool(count_only)), sparse=int(bool(sparse)), allow_full=int(bool(allow_full)), n_queries=len(queries))
        for k, (qk, qn) in enumerate(queries):
            d.query_key[k] = int(qk)
            d.query_need[k] = int(qn)
        cap = H * W // 4 + (H + W) // 2 + 4
        bufs = dict(root=np.empty((n, H, W), np.int32), area=np.empty((n, H, W), np.uint32), sumy=np.empty((n, H, W), np.uint64),
                    sumx=np.empty((n, H, W), np.uint64), flag=np.empty((n, H, W), np.uint32), counters=np.empty((n, 16), np.int32),
                    list1=np.empty((n, cap), np.int32), list2=np.empty((n, cap), np.int32),
                    tile_any=np.empty((n, (H + 31) // 32, (W + 63) // 64), np.uint8))
        o = CclPassOut(**{k: v.ctypes.data for k, v in bufs.items()})
        self._check(self.lib.ecseg_ccl_pass_debug(self.h, _ptr(a), _ptr(x), n, H, W, C.byref(d), C.byref(o)), 'ecseg_ccl_pass_debug')
        cnt = bufs.pop('counters')
        l1, l2 = bufs.pop('list1'), bufs.pop('list2')
        bufs.update(ncomp=cnt[:, 0:3].copy(), npx=cnt[:, 3:6].copy(), last_root=cnt[:, 6].copy(), nlist1=cnt[:, 7].copy(),
                    nlist2=cnt[:, 8].copy(), cnt=cnt[:, 9:14].copy(),
                    list1=[l1[i, :max(0, min(cap, int(cnt[i, 7])))].copy() for i in range(n)],
                    list2=[l2[i, :max(0, min(cap, int(cnt[i, 8])))].copy() for i in range(n)])
        return bufs

    def scratch_fill_debug(self, byte):
        """Test-only (ecseg_scratch_fill_debug): fills the whole capacity of every scratch arena of the handle with ``byte`` (0 .. 255),
        between two waits for the handle's streams.  The region map of ``nuclei_regions``, what was sent or decoded ahead and the
        clean-up workspace's layout are withdrawn; every driver must answer afterwards as on a fresh handle."""
        self._check(self.lib.ecseg_scratch_fill_debug(self.h, int(byte)), 'ecseg_scratch_fill_debug')

    def count_colocalization(self, ob1, ob2):
        a, single = self._stack(ob1)
        b, _ = self._stack(ob2)
        n, H, W = a.shape
        cnt = np.zeros(n, np.int32)
        self._check(self.lib.ecseg_count_colocalization(self.h, _ptr(a), _ptr(b), n, H, W, _ptr(cnt)),
                    'ecseg_count_colocalization')
        return int(cnt[0]) if single else cnt

    def count_hsr(self, chrom, fish, size_threshold=20):
        a, single = self._stack(chrom)
        b, _ = self._stack(fish)
        n, H, W = a.shape
        cnt = np.zeros(n, np.int32)
        self._check(self.lib.ecseg_count_hsr(self.h, _ptr(a), _ptr(b), n, H, W, int(size_threshold), _ptr(cnt)),
                    'ecseg_count_hsr')
        return int(cnt[0]) if single else cnt

    def overlay(self, labels, rgb, sensitivity, hsr_size_threshold=20):
        a, single = self._stack(labels)
        r = _u8(rgb)
        if r.ndim == 3:
            r = r[None]
        n, H, W = a.shape
        if r.shape[:3] != (n, H, W) or r.shape[3] < 2:
            raise ValueError('rgb must be (n, H, W, C>=2) matching labels')
        out = np.zeros((n, 12), np.int64)
        self._check(self.lib.ecseg_overlay(self.h, _ptr(a), _ptr(r), n, H, W, r.shape[3], int(sensitivity),
                                           int(hsr_size_threshold), _ptr(out)), 'ecseg_overlay')
        return out[0] if single else out

    # ---- interSeg driver ------------------------------------------------------------------------------
    def nuclei_regions(self, seg, img, channel0, capacity=4096):
        """(H, W) uint8 nucleus mask + (>= H, >= W, C) uint8 image -> int64 (n_regions, 8) records (ecseg_nuclei_regions): area,
        bbox (min row, min col, max row + 1, max col + 1), sum of rows, sum of columns, sum of channel ``channel0``.  The region
        map stays on the handle for ``nucleus_crops``."""
        s = _u8(seg)
        im = _u8(img)
        if s.ndim != 2 or im.ndim != 3:
            raise ValueError('nuclei_regions takes a (H, W) mask and an (H, W, C) image')
        H, W = s.shape
        n = C.c_int32()
        cap = int(capacity)
        while True:
            rec = np.empty((max(cap, 1), 8), np.int64)
            self._check(self.lib.ecseg_nuclei_regions(self.h, _ptr(s), H, W, _ptr(im), im.shape[0], im.shape[1], im.shape[2],
                                                      int(channel0), cap, _ptr(rec), C.byref(n)), 'ecseg_nuclei_regions')
            if n.value <= cap:
                return rec[:n.value]
            cap = n.value

    def nucleus_crops(self, crops, channel_order=(0, 1, 2)):
        """(N, 5) int32 (region, y0, x0, h, w) windows of the last ``nuclei_regions`` image -> (uint8 (N, 256, 256, 3) crops,
        int32 (N, 3) per-channel maxima) (ecseg_nucleus_crops)."""
        d = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
        order = np.ascontiguousarray(channel_order, np.int32)
        out = np.empty((len(d), 256, 256, 3), np.uint8)
        mx = np.zeros((len(d), 3), np.int32)
        self._check(self.lib.ecseg_nucleus_crops(self.h, _ptr(d), len(d), _ptr(order), _ptr(out), _ptr(mx)), 'ecseg_nucleus_crops')
        return out, mx

    def classify_nucleus_crops(self, desc, order, from_patches, centromeric, model_i, model_c=None, want_crops=False, pred_i=None,
                               pred_c=None):
        """The crops of ``nucleus_crops`` through the two classifiers without leaving the device (ecseg_classify_nucleus_crops).
        ``from_patches``: a bool or one per crop; ``centromeric``: ecSeg-c applies to this image; ``model_i`` / ``model_c``: a
        ``Handle`` with the plan loaded, or an object holding one as ``.handle`` (``model_i`` may be this handle's own).  Returns
        (channel_max int32 (N, 3), pred_i float32 (N, 3), ran_i bool (N), pred_c float32 (N), ran_c bool (N)[, crops uint8
        (N, 256, 256, 3) with ``want_crops``]); the rows of ``pred_i`` / ``pred_c`` whose ``ran_*`` is false are not written - zeros,
        or what the arrays given as ``pred_i`` / ``pred_c`` held."""
        d = np.ascontiguousarray(desc, np.int32).reshape(-1, 5)
        n = len(d)
        order = np.ascontiguousarray(order, np.int32)
        if order.shape != (3,):
            raise ValueError('channel order must hold 3 channels')
        fp = np.ascontiguousarray(np.broadcast_to(np.asarray(from_patches, bool), (n,))).view(np.uint8)
        hi = getattr(model_i, 'handle', model_i)
        hc = getattr(model_c, 'handle', model_c)
        mx = np.zeros((n, 3), np.int32)
        pi = np.zeros((n, 3), np.float32) if pred_i is None else pred_i
        pc = np.zeros(n, np.float32) if pred_c is None else pred_c
        for a, shape in ((pi, (n, 3)), (pc, (n,))):
            if a.dtype != np.float32 or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError('pred_i / pred_c must be C-contiguous float32 arrays of shape (N, 3) / (N,)')
        ri, rc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        crops = np.empty((n, 256, 256, 3), np.uint8) if want_crops else None
        self._check(self.lib.ecseg_classify_nucleus_crops(self.h, hi.h, hc.h if hc is not None else None, _ptr(d), n, _ptr(order), _ptr(fp),
                                                          int(bool(centromeric)), _ptr(mx), _ptr(pi), _ptr(ri), _ptr(pc), _ptr(rc), _ptr(crops)),
                    'ecseg_classify_nucleus_crops')
        out = (mx, pi, ri.view(bool), pc, rc.view(bool))
        return out + (crops,) if want_crops else out

    ISEG_OK, ISEG_INSTANCE_IDS, ISEG_RECORDS_OVERFLOW, ISEG_CROPS_OVERFLOW = 0, 1, 2, 3       # ECSEG_ISEG_* of the header

    def interseg_batch_packed(self, packed, table, fish_index, model_i, model_c, record_capacity, crop_capacity):
        """ecseg_interseg_batch as the header states it: a uint8 buffer, its (n, 8) int64 table (image offset, H, W, C, segmentation
        offset, h, w, run_c) and the two capacities -> (out int32 (n, 8), records int64 (record_capacity, 8), and per crop
        (crop_capacity entries each) crop_region int32, channel_max int32 (., 3), pred_i float32 (., 3), ran_i bool, pred_c float32,
        ran_c bool).  ``interseg_many`` packs, sizes and unpacks for its caller."""
        buf = _u8(packed).reshape(-1)
        tab = np.ascontiguousarray(table, np.int64).reshape(-1, 8)
        rcap, ccap = int(record_capacity), int(crop_capacity)
        hi = getattr(model_i, 'handle', model_i)
        hc = getattr(model_c, 'handle', model_c)
        out = np.zeros((len(tab), 8), np.int32)
        rec = np.zeros((max(rcap, 1), 8), np.int64)
        region, mx = np.zeros(max(ccap, 1), np.int32), np.zeros((max(ccap, 1), 3), np.int32)
        pi, pc = np.zeros((max(ccap, 1), 3), np.float32), np.zeros(max(ccap, 1), np.float32)
        ri, rc = np.zeros(max(ccap, 1), np.uint8), np.zeros(max(ccap, 1), np.uint8)
        self._check(self.lib.ecseg_interseg_batch(self.h, hi.h, hc.h if hc is not None else None, _ptr(buf), buf.size, _ptr(tab), len(tab),
                                                  int(fish_index), rcap, ccap, _ptr(out), _ptr(rec), _ptr(region), _ptr(mx), _ptr(pi), _ptr(ri),
                                                  _ptr(pc), _ptr(rc)), 'ecseg_interseg_batch')
        return out, rec[:rcap], region[:ccap], mx[:ccap], pi[:ccap], ri[:ccap].view(bool), pc[:ccap], rc[:ccap].view(bool)

    def interseg_many(self, images, segs, fish_index, quality_pass, model_i, model_c=None, record_capacity=None, crop_capacity=None):
        """``nuclei_regions`` + the crop windows of ``interseg.region_rows`` + ``classify_nucleus_crops`` for a list of images in one
        device call (ecseg_interseg_batch).  ``images``: (H, W, C >= 3) uint8 each; ``segs``: their (h, w) uint8 masks, not larger than
        their image; ``quality_pass``: one bool per image, ecSeg-c applies to an image only where it is true (and ``model_c`` is given).
        Returns one entry per image: ``(records int64 (n, 8), (owner int64, pred_i float32 (N, 3), ran_i bool, pred_c float32, ran_c
        bool))`` with N the image's crops and ``owner`` their regions, or the ``EcsegError`` (code -1) ``nuclei_regions`` raises for
        that image alone - an instance-id map.  ``record_capacity`` / ``crop_capacity``: room for the first call (default 1024 records
        and 512 crops per image); the images reported as not fitting go again, together, with the room they asked for."""
        n = len(images)
        if not (len(segs) == n == len(quality_pass)):
            raise ValueError('interseg_many takes one segmentation and one quality_pass flag per image')
        ims = [_u8(a) for a in images]
        sgs = [_u8(a) for a in segs]
        for im, sg in zip(ims, sgs):
            if im.ndim != 3 or sg.ndim != 2:
                raise ValueError('interseg_many takes (H, W, C) images and (h, w) masks')
        results = [None] * n
        todo = list(range(n))
        rcap = int(record_capacity) if record_capacity is not None else 1024 * n
        ccap = int(crop_capacity) if crop_capacity is not None else 512 * n
        while todo:
            parts, tab, off = [], np.zeros((len(todo), 8), np.int64), 0
            for j, i in enumerate(todo):
                im, sg = ims[i], sgs[i]
                tab[j] = (off, im.shape[0], im.shape[1], im.shape[2], off + im.size, sg.shape[0], sg.shape[1], int(bool(quality_pass[i])))
                parts += [im.reshape(-1), sg.reshape(-1)]
                off += im.size + sg.size
            out, rec, region, _, pi, ri, pc, rc = self.interseg_batch_packed(np.concatenate(parts), tab, fish_index, model_i, model_c, rcap, ccap)
            again, need_r, need_c = [], 0, 0
            for j, i in enumerate(todo):
                st, nr, r0, ncr, c0, vmin, vmax = (int(v) for v in out[j, :7])
                if st == self.ISEG_INSTANCE_IDS:
                    e = EcsegError('ecseg_nuclei_regions failed (-1): segmentation holds the non-zero values %d .. %d: only 0 / non-zero '
                                   'nucleus masks are supported, not instance-id maps' % (vmin, vmax))
                    e.code = -1
                    results[i] = e
                elif st == self.ISEG_OK:
                    sl = slice(c0, c0 + ncr)
                    results[i] = (rec[r0:r0 + nr].copy(), (region[sl].astype(np.int64), pi[sl].copy(), ri[sl].copy(), pc[sl].copy(), rc[sl].copy()))
                else:
                    again.append(i)
                    need_r += nr
                    need_c += max(ncr, 512)                   # (-1: not counted yet, the next round says)
            if again and len(again) == len(todo) and need_r <= rcap and need_c <= ccap:
                raise EcsegError('ecseg_interseg_batch: image %d fits neither %d records nor %d crops' % (again[0], rcap, ccap))
            todo, rcap, ccap = again, max(rcap, need_r), max(ccap, need_c)
        return results

    def iseg_classifier_inputs(self, crops, channel_max, sel_i, sel_c):
        """The input kernel of ``classify_nucleus_crops`` alone, for its tests (ecseg_iseg_classifier_inputs_debug): uint8 (k, 256, 256, 3)
        crops with their (k, 3) maxima and two lists of crop indices -> (float32 (len(sel_i), 256, 256, 1), float32 (len(sel_c), 256,
        256, 3))."""
        c = _u8(crops)
        if c.ndim != 4 or c.shape[1:] != (256, 256, 3):
            raise ValueError('crops must be (k, 256, 256, 3) uint8')
        mx = np.ascontiguousarray(channel_max, np.int32).reshape(len(c), 3)
        si, sc = np.ascontiguousarray(sel_i, np.int32).reshape(-1), np.ascontiguousarray(sel_c, np.int32).reshape(-1)
        oi, oc = np.empty((len(si), 256, 256, 1), np.float32), np.empty((len(sc), 256, 256, 3), np.float32)
        self._check(self.lib.ecseg_iseg_classifier_inputs_debug(self.h, _ptr(c), len(c), _ptr(mx), _ptr(si), len(si), _ptr(sc), len(sc), _ptr(oi),
                                                                _ptr(oc)), 'ecseg_iseg_classifier_inputs_debug')
        return oi, oc

    # ---- fish_distance_calculation -----------------------------------------------------------------------
    def fish_distances(self, labels, lsq, fish_channel, centromere_channel, capacity=4096):
        """(H, W) int32 instance labels (<= 0 background) + (H, W, C >= 2) uint8 lsq image -> int64 (n_cells, 8) records in
        ascending label order (ecseg_fish_distances): label, area, gate bits, FISH pixels, centromere pixels, FISH components,
        min squared FISH - centromere distance (-1: a set is empty), 0."""
        lab = np.ascontiguousarray(labels)
        if lab.dtype != np.int32:
            if lab.dtype.kind not in 'iu' or (lab.size and (int(lab.max()) > 2 ** 31 - 1 or int(lab.min()) < -2 ** 31)):
                raise ValueError('fish_distances takes integer labels that fit int32')
            lab = lab.astype(np.int32)
        im = _u8(lsq)
        if lab.ndim != 2 or im.ndim != 3 or im.shape[:2] != lab.shape:
            raise ValueError('fish_distances takes a (H, W) label map and an (H, W, C) image of the same extent')
        H, W = lab.shape
        n = C.c_int32()
        cap = int(capacity)
        while True:
            rec = np.empty((max(cap, 1), 8), np.int64)
            self._check(self.lib.ecseg_fish_distances(self.h, _ptr(lab), H, W, _ptr(im), im.shape[2], int(fish_channel),
                                                      int(centromere_channel), cap, _ptr(rec), C.byref(n)), 'ecseg_fish_distances')
            if n.value <= cap:
                return rec[:n.value]
            cap = n.value

    FISH_DISTANCES_BATCH_MAX_IMAGES = 8192

    def fish_distances_batch_raw(self, labels, lsqs, fish_channel, centromere_channel, record_capacity):
        """ecseg_fish_distances_batch as it is: contiguous (H, W) int32 label maps and (H, W, C) uint8 images -> (records int64
        (record_capacity, 8) - written only when the chunk's cells fit -, n_cells (n,) int32, status (n,) int32)."""
        n = len(labels)
        shapes = np.zeros((max(n, 1), 3), np.int32)
        for i, im in enumerate(lsqs):
            shapes[i] = im.shape
        cap = int(record_capacity)
        rec = np.zeros((max(cap, 1), 8), np.int64)
        n_cells, status = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        lp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in labels])
        ip = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in lsqs])
        self._check(self.lib.ecseg_fish_distances_batch(self.h, n, lp, ip, _ptr(shapes), int(fish_channel), int(centromere_channel), cap,
                                                        _ptr(rec), _ptr(n_cells), _ptr(status)), 'ecseg_fish_distances_batch')
        return rec[:cap], n_cells[:n], status[:n]

    def fish_distances_many(self, labels, lsqs, fish_channel, centromere_channel, record_capacity=4096):
        """``fish_distances`` for a list of images of any extents in one device call (ecseg_fish_distances_batch).  Returns one entry
        per image: the int64 (n_cells, 8) records ``fish_distances`` returns, or the ``EcsegError`` (code -1) it raises for that image
        alone - a label above H * W.  The error is returned, not raised: the other images of the chunk keep their answers.
        ``record_capacity``: room for the records of the whole chunk on the first call; a chunk holding more goes once more with the
        room it reported.  Lists longer than ``FISH_DISTANCES_BATCH_MAX_IMAGES`` go in several calls."""
        if len(labels) != len(lsqs):
            raise ValueError('fish_distances_many takes one lsq image per label map')
        labs, ims = [], []
        for lab, im in zip(labels, lsqs):
            lab = np.ascontiguousarray(lab)
            if lab.dtype != np.int32:
                if lab.dtype.kind not in 'iu' or (lab.size and (int(lab.max()) > 2 ** 31 - 1 or int(lab.min()) < -2 ** 31)):
                    raise ValueError('fish_distances_many takes integer labels that fit int32')
                lab = lab.astype(np.int32)
            im = _u8(im)
            if lab.ndim != 2 or im.ndim != 3 or im.shape[:2] != lab.shape:
                raise ValueError('fish_distances_many takes (H, W) label maps and (H, W, C) images of the same extent')
            labs.append(lab)
            ims.append(im)
        out = []
        for i0 in range(0, len(labs), self.FISH_DISTANCES_BATCH_MAX_IMAGES):
            sl = slice(i0, i0 + self.FISH_DISTANCES_BATCH_MAX_IMAGES)
            cap = int(record_capacity)
            rec, n_cells, status = self.fish_distances_batch_raw(labs[sl], ims[sl], fish_channel, centromere_channel, cap)
            if int(n_cells.sum()) > cap:
                cap = int(n_cells.sum())
                rec, n_cells, status = self.fish_distances_batch_raw(labs[sl], ims[sl], fish_channel, centromere_channel, cap)
            at = 0
            for lab, k, st in zip(labs[sl], n_cells.tolist(), status.tolist()):
                if st != 0:
                    e = EcsegError('ecseg_fish_distances failed (%d): fish_distances: the label map holds a label larger than H * W = %d '
                                   '(renumber the labels by rank first)' % (st, lab.size))
                    e.code = st
                    out.append(e)
                else:
                    out.append(rec[at:at + k].copy())
                at += k
        return out

    # ---- stat_fish -------------------------------------------------------------------------------------
    FISH_SPOT_INT64 = 24

    def fish_spots(self, labels, img, probe_channels, weights, normal_threshold, intensity_thresholds, min_cc_size, line_thickness,
                   capacity=4096):
        """(H, W) int32 instance labels (<= 0 background) + (H, W, C) uint8 image -> (int64 (n_cells, 24) records in ascending
        label order, cleaned thresholded masks uint8 (H, W, n_probe), boundaries uint8 (H, W)) (ecseg_fish_spots; the record
        layout is in include/ecseg_hip.h).  ``weights``: the K x K float64 projected Gaussian kernel, K odd."""
        lab = np.ascontiguousarray(labels)
        if lab.dtype != np.int32:
            if lab.dtype.kind not in 'iu' or (lab.size and (int(lab.max()) > 2 ** 31 - 1 or int(lab.min()) < -2 ** 31)):
                raise ValueError('fish_spots takes integer labels that fit int32')
            lab = lab.astype(np.int32)
        im = _u8(img)
        if lab.ndim != 2 or im.ndim != 3 or im.shape[:2] != lab.shape:
            raise ValueError('fish_spots takes a (H, W) label map and an (H, W, C) image of the same extent')
        ch = np.ascontiguousarray(probe_channels, np.int32).reshape(-1)
        thr_in = np.ascontiguousarray(intensity_thresholds, np.float64).reshape(-1)
        w = np.ascontiguousarray(weights, np.float64)
        if w.ndim != 2 or w.shape[0] != w.shape[1]:
            raise ValueError('fish_spots takes a square K x K kernel')
        if len(thr_in) != len(ch):
            raise ValueError('fish_spots takes one intensity threshold per probe channel')
        H, W = lab.shape
        n = C.c_int32()
        cap = int(capacity)
        thr = np.empty((H, W, max(len(ch), 1)), np.uint8)
        bnd = np.empty((H, W), np.uint8)
        while True:
            rec = np.empty((max(cap, 1), self.FISH_SPOT_INT64), np.int64)
            self._check(self.lib.ecseg_fish_spots(self.h, _ptr(lab), H, W, _ptr(im), im.shape[2], _ptr(ch), len(ch), _ptr(w), w.shape[0],
                                                  float(normal_threshold), _ptr(thr_in), int(min_cc_size), int(line_thickness), cap,
                                                  _ptr(thr), _ptr(bnd), _ptr(rec), C.byref(n)), 'ecseg_fish_spots')
            if n.value <= cap:
                return rec[:n.value], thr, bnd
            cap = n.value

    def fish_render(self, img, channels, thresholded, boundaries):
        """(H, W, C) uint8 image, C = 3 or 4, with ``channels`` = the indices of its blue, green, red (and aqua) channel + the
        (H, W, C - 1) masks and (H, W) boundaries of ``fish_spots`` -> the three (H, W, 3) uint8 RGB rasters stat_fish writes:
        ``_original``, ``_original_with_segmentation`` and ``_lsq_`` (ecseg_fish_render; the rules are in include/ecseg_hip.h)."""
        im, thr, bnd = _u8(img), _u8(thresholded), _u8(boundaries)
        if im.ndim != 3 or thr.ndim != 3 or bnd.ndim != 2 or thr.shape[:2] != im.shape[:2] or bnd.shape != im.shape[:2]:
            raise ValueError('fish_render takes an (H, W, C) image, (H, W, n_probe) masks and (H, W) boundaries of one extent')
        ch = np.ascontiguousarray(channels, np.int32).reshape(-1)
        if len(ch) != im.shape[2]:
            raise ValueError('fish_render takes one channel index per image channel (blue, green, red[, aqua])')
        H, W = bnd.shape
        out = [np.empty((H, W, 3), np.uint8) for _ in range(3)]
        self._check(self.lib.ecseg_fish_render(self.h, _ptr(im), H, W, im.shape[2], _ptr(ch), _ptr(thr), thr.shape[2], _ptr(bnd),
                                               _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), 'ecseg_fish_render')
        return tuple(out)

    def tiff_encode(self, img, invert=False, capacity=None):
        """(H, W) or (H, W, 3) uint8 image -> the bytes of the file ``image_io.write_tiff_gray8(path, img, invert)`` /
        ``write_tiff_rgb8(path, img)`` writes, with every LZW strip encoded on the device (ecseg_tiff_encode).  ``capacity``: bytes
        of the buffer the file is built in, by default ecseg_tiff_encode_bound; a file that does not fit raises, with code -1."""
        im = _u8(img)
        if im.ndim == 3 and im.shape[2] == 1:
            im = im[..., 0]
        if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3) or not im.size:
            raise ValueError('tiff_encode takes a non-empty (H, W) or (H, W, 3) uint8 image')
        H, W = im.shape[:2]
        spp = 1 if im.ndim == 2 else 3
        cap = self.lib.ecseg_tiff_encode_bound(H, W, spp) if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError('tiff_encode: an image of %d x %d x %d samples cannot be written as a TIFF' % (H, W, spp))
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_longlong()
        self._check(self.lib.ecseg_tiff_encode(self.h, _ptr(im), H, W, spp, int(bool(invert)), _ptr(out), cap, C.byref(n)), 'ecseg_tiff_encode')
        return out[:n.value].tobytes()

    tiff_options = tiff_options

    @property
    def tiff_kinds(self):
        """The kinds of file ``tiff_decode`` and ``tiff_decode_many`` take now, as the word of the routing functions."""
        return tiff_kinds(self.tiff_deflate_on_device, self.tiff_tiled_on_device, self.tiff_packbits_on_device)

    def tiff_decode(self, data, deflate=None):
        """The bytes of a TIFF file -> what ``image_io.read_tiff`` returns for that file, (H, W) or (H, W, spp) uint8 / uint16, with
        every strip decoded on the device (ecseg_tiff_decode); None for a file that is left to the host readers (ECSEG_E_UNSUPPORTED:
        BigTIFF, Deflate, and tiles or PackBits unless the handle option ``tiff_tiled_on_device`` / ``tiff_packbits_on_device`` is on).  Whether a file is worth sending here is ``image_io.imread``'s question (ecseg_tiff_decode_routes).  A corrupt file raises, with code -1.
        ``deflate``: True / False: the call runs with the handle option ``tiff_deflate_on_device`` on / off - on, Deflate strips
        (compression 8 and 32946) are decoded too, and such a file is an array or an error, not None; None: as the option stands."""
        with self.tiff_options(deflate=deflate):
            return self._tiff_decode(data)

    def _tiff_decode(self, data):
        buf = _file_u8(data)
        H, W, spp, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        shape = (C.byref(H), C.byref(W), C.byref(spp), C.byref(bits))
        rc = self.lib.ecseg_tiff_decode(self.h, _ptr(buf), buf.size, None, 0, *shape)
        if rc == E_UNSUPPORTED:
            return None
        self._check(rc, 'ecseg_tiff_decode')
        out = np.empty((H.value, W.value, spp.value), np.uint8 if bits.value == 8 else np.uint16)
        rc = self.lib.ecseg_tiff_decode(self.h, _ptr(buf), buf.size, _ptr(out), out.nbytes, *shape)
        if rc == E_UNSUPPORTED:
            return None
        self._check(rc, 'ecseg_tiff_decode')
        return out[..., 0] if spp.value == 1 else out

    def tiff_decode_packed(self, files, ranges, dst=None, dst_offsets=None):
        """ecseg_tiff_decode_batch as it is: ``files`` a 1-D uint8 buffer, ``ranges`` (n, 2) int64 rows (byte offset, bytes) -> (shapes
        (n, 4) int32: H, W, samples per pixel, bits; status (n,) int32).  ``dst``: a 1-D uint8 buffer that receives the raster of file i
        at ``dst_offsets[i]``; without it only shapes and status are filled."""
        buf = np.ascontiguousarray(files, np.uint8).reshape(-1)
        tab = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
        shapes, status = np.zeros((len(tab), 4), np.int32), np.zeros(len(tab), np.int32)
        offs = None if dst_offsets is None else np.ascontiguousarray(dst_offsets, np.int64).reshape(-1)
        if dst is not None and (offs is None or len(offs) != len(tab) or dst.dtype != np.uint8 or dst.ndim != 1 or not dst.flags.c_contiguous):
            raise ValueError('tiff_decode_packed takes a 1-D uint8 destination and one offset per file')
        self._check(self.lib.ecseg_tiff_decode_batch(self.h, _ptr(buf), buf.size, _ptr(tab), len(tab), _ptr(dst), 0 if dst is None else dst.size,
                                                     _ptr(offs), _ptr(shapes), _ptr(status)), 'ecseg_tiff_decode_batch')
        return shapes, status

    def tiff_decode_many(self, datas, budget_bytes=8 << 30, deflate=None):
        """``tiff_decode`` over a list of files at once (ecseg_tiff_decode_batch: a wave per strip, the strips of all files side by side).
        -> a list with, per file, the array ``tiff_decode`` returns for it alone, None where it returns None, or the error it raises -
        returned in its place, not raised (``segment_many``'s rule), so that one bad file costs the others nothing.  The files are packed
        back to back (``pack_file_images``) and go in one call while the sum of what ecseg_tiff_decode_batch_bytes says each needs
        stays within ``budget_bytes`` of device scratch, else in several calls over consecutive files; a file that exceeds the budget
        alone goes alone.  ``deflate``: as in ``tiff_decode``."""
        with self.tiff_options(deflate=deflate):
            return self._tiff_decode_many(datas, budget_bytes)

    def _tiff_decode_many(self, datas, budget_bytes):
        out = [None] * len(datas)
        todo = []                                              # (position, bytes as uint8)
        for k, data in enumerate(datas):
            try:
                todo.append((k, _file_u8(data)))
            except (TypeError, ValueError) as e:
                out[k] = e

        if not todo:
            return out
        buf, ranges = pack_file_images([b for _, b in todo])     # packed once: every call reads its files through its rows of the table
        # what each file needs alone, asked once per file: their sum is at least what a call over them needs (every slot rounds up alone)
        needs = [self.lib.ecseg_tiff_decode_batch_bytes(_ptr(buf), buf.size, _ptr(np.ascontiguousarray(ranges[k:k + 1])), 1, self.tiff_kinds)
                 for k in range(len(todo))]
        chunks, lo, held = [], 0, 0
        for hi, need in enumerate(needs):
            if hi > lo and (need < 0 or held < 0 or held + need > budget_bytes):
                chunks.append((lo, hi))
                lo, held = hi, 0
            held = -1 if need < 0 or held < 0 else held + need
        chunks.append((lo, len(todo)))
        for lo, hi in chunks:
            chunk, tab = todo[lo:hi], ranges[lo:hi]
            shapes, status = self.tiff_decode_packed(buf, tab)
            sizes = [int(H) * W * spp * (bits // 8) if st == 0 else 0 for (H, W, spp, bits), st in zip(shapes.tolist(), status.tolist())]
            offs, end = [], 0
            for (H, W, spp, bits), n in zip(shapes.tolist(), sizes):
                end += end & 1 if bits == 16 else 0                # a 16-bit raster starts on an even byte
                offs.append(end)
                end += n
            dst = np.empty(max(end, 1), np.uint8)
            if end:
                _, status = self.tiff_decode_packed(buf, tab, dst, offs)
            for (k, _), (H, W, spp, bits), st, off, n in zip(chunk, shapes.tolist(), status.tolist(), offs, sizes):
                if st == E_UNSUPPORTED:
                    out[k] = None
                elif st != 0:
                    out[k] = EcsegError('ecseg_tiff_decode failed (%d): file %d of the batch is not a TIFF file, or a corrupt one' % (st, k))
                    out[k].code = st
                else:
                    a = dst[off:off + n].view(np.uint8 if bits == 8 else np.uint16).reshape(H, W, spp)
                    out[k] = a[..., 0] if spp == 1 else a
        return out

    def fish_render_tiff(self, img, channels, thresholded, boundaries, want_rasters=False):
        """``fish_render``'s inputs -> the bytes of the three files ``image_io.write_tiff_rgb8`` writes for its rasters (``_original``,
        ``_original_with_segmentation``, ``_lsq_``): rendered and LZW-encoded without leaving the device (ecseg_fish_render_tiff).
        ``want_rasters``: return (files, rasters), the rasters as ``fish_render`` returns them."""
        im, thr, bnd = _u8(img), _u8(thresholded), _u8(boundaries)
        if im.ndim != 3 or thr.ndim != 3 or bnd.ndim != 2 or thr.shape[:2] != im.shape[:2] or bnd.shape != im.shape[:2]:
            raise ValueError('fish_render_tiff takes an (H, W, C) image, (H, W, n_probe) masks and (H, W) boundaries of one extent')
        ch = np.ascontiguousarray(channels, np.int32).reshape(-1)
        if len(ch) != im.shape[2]:
            raise ValueError('fish_render_tiff takes one channel index per image channel (blue, green, red[, aqua])')
        H, W = bnd.shape
        cap = self.lib.ecseg_tiff_encode_bound(H, W, 3)
        if cap < 0:
            raise ValueError('fish_render_tiff: an image of %d x %d pixels cannot be written as a TIFF' % (H, W))
        files = [np.empty(cap, np.uint8) for _ in range(3)]
        ptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in files])
        n = (C.c_longlong * 3)()
        rasters = [np.empty((H, W, 3), np.uint8) for _ in range(3)] if want_rasters else [None] * 3
        self._check(self.lib.ecseg_fish_render_tiff(self.h, _ptr(im), H, W, im.shape[2], _ptr(ch), _ptr(thr), thr.shape[2], _ptr(bnd), ptrs, cap, n,
                                                    *[_ptr(r) if r is not None else None for r in rasters]), 'ecseg_fish_render_tiff')
        out = tuple(f[:k].tobytes() for f, k in zip(files, n))
        return (out, tuple(rasters)) if want_rasters else out

    def tiff_encode_packed(self, rasters, table, capacity=None):
        """ecseg_tiff_encode_batch as it is: ``rasters`` a 1-D uint8 buffer, ``table`` (n, 5) int64 rows (byte offset, H, W, spp,
        invert) -> (out, ranges): a 1-D uint8 buffer with the file images back to back and (n, 2) int64 rows (offset, bytes) into it.
        ``capacity``: bytes of ``out``, by default the sum of ecseg_tiff_encode_bound over the rows (rows the bound refuses count as
        nothing: the call refuses them itself)."""
        buf = np.ascontiguousarray(rasters, np.uint8).reshape(-1)
        tab = np.ascontiguousarray(table, np.int64).reshape(-1, 5)
        if capacity is None:
            i32 = lambda v: int(min(max(v, -1), 2 ** 31 - 1))
            capacity = sum(max(self.lib.ecseg_tiff_encode_bound(i32(H), i32(W), i32(spp)), 0) for _, H, W, spp, _ in tab.tolist())
        out = np.empty(max(int(capacity), 1), np.uint8)
        ranges = np.zeros((len(tab), 2), np.int64)
        self._check(self.lib.ecseg_tiff_encode_batch(self.h, _ptr(buf), buf.size, _ptr(tab), len(tab), _ptr(out), int(capacity), _ptr(ranges)),
                    'ecseg_tiff_encode_batch')
        return out, ranges

    @staticmethod
    def _split_by_budget(needs, budget_bytes):
        """Consecutive (lo, hi) chunks of a list whose needs stay within the budget; an item that exceeds it alone goes alone
        (``tiff_decode_many``'s rule; a negative need - an item its call will refuse - goes alone too)."""
        chunks, lo, held = [], 0, 0
        for hi, need in enumerate(needs):
            if hi > lo and (need < 0 or held < 0 or held + need > budget_bytes):
                chunks.append((lo, hi))
                lo, held = hi, 0
            held = -1 if need < 0 or held < 0 else held + need
        if needs:
            chunks.append((lo, len(needs)))
        return chunks

    def tiff_encode_many(self, rasters, inverts=None, budget_bytes=8 << 30):
        """``tiff_encode`` over a list of (H, W) / (H, W, 3) uint8 images at once (ecseg_tiff_encode_batch: a wave per strip, the
        strips of all files side by side) -> the list of their files as ``bytes``, in input order, each what ``tiff_encode`` returns
        for that image alone.  ``inverts``: one flag per image (default: none inverted).  The images go in one call while the sum of
        what ecseg_tiff_encode_batch_bytes says each needs stays within ``budget_bytes`` of device scratch, else in several calls over
        consecutive images; an image that exceeds the budget alone goes alone."""
        ims = []
        for img in rasters:
            im = _u8(img)
            if im.ndim == 3 and im.shape[2] == 1:
                im = im[..., 0]
            if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3) or not im.size:
                raise ValueError('tiff_encode_many takes non-empty (H, W) or (H, W, 3) uint8 images')
            ims.append(im)
        inverts = [False] * len(ims) if inverts is None else [bool(v) for v in inverts]
        if len(inverts) != len(ims):
            raise ValueError('tiff_encode_many takes one invert flag per image')
        rows = [[0, im.shape[0], im.shape[1], 1 if im.ndim == 2 else 3, int(v)] for im, v in zip(ims, inverts)]
        needs = [self.lib.ecseg_tiff_encode_batch_bytes(_ptr(np.array(r, np.int64)), 1) for r in rows]
        out = []
        for lo, hi in self._split_by_budget(needs, budget_bytes):
            tab, end = np.array(rows[lo:hi], np.int64), 0
            for k, im in enumerate(ims[lo:hi]):
                tab[k, 0] = end
                end += im.size
            buf = np.empty(end, np.uint8)
            for k, im in enumerate(ims[lo:hi]):
                buf[tab[k, 0]:tab[k, 0] + im.size] = im.reshape(-1)
            files, ranges = self.tiff_encode_packed(buf, tab)
            out += [files[o:o + n].tobytes() for o, n in ranges.tolist()]
        return out

    def fish_render_tiff_many(self, items, budget_bytes=8 << 30):
        """``fish_render_tiff`` over a list of images at once, with the other TIFF files of each image (ecseg_fish_render_tiff_batch):
        ``items`` is a list of (img, channels, thresholded, boundaries, mask, picture) - the first four as ``fish_render_tiff`` takes
        them, ``mask`` an (H, W) uint8 raster or None, ``picture`` an (H, W, 3) uint8 raster or None - -> per item the tuple (original,
        with_segmentation, lsq, mask file or None, picture file or None) of ``bytes``, each what ``fish_render_tiff`` and
        ``tiff_encode`` return for it alone.  All files of all items of a call go through one batched encode; the items are split
        into consecutive calls by ``budget_bytes`` of device scratch as ``tiff_encode_many`` splits its list."""
        prepared, needs = [], []
        for item in items:
            img, channels, thresholded, boundaries, mask, picture = item
            im, thr, bnd = _u8(img), _u8(thresholded), _u8(boundaries)
            if im.ndim != 3 or thr.ndim != 3 or bnd.ndim != 2 or thr.shape[:2] != im.shape[:2] or bnd.shape != im.shape[:2]:
                raise ValueError('fish_render_tiff_many takes (H, W, C) images, (H, W, n_probe) masks and (H, W) boundaries of one extent')
            ch = np.ascontiguousarray(channels, np.int32).reshape(-1)
            if len(ch) != im.shape[2] or thr.shape[2] != im.shape[2] - 1 or not 3 <= len(ch) <= 4:
                raise ValueError('fish_render_tiff_many takes one channel index per image channel (blue, green, red[, aqua]) and one mask per probe')
            H, W = bnd.shape
            m = None if mask is None else _u8(mask)
            p = None if picture is None else _u8(picture)
            if (m is not None and m.shape != (H, W)) or (p is not None and p.shape != (H, W, 3)):
                raise ValueError('fish_render_tiff_many takes an (H, W) mask and an (H, W, 3) picture of the image\'s extent, or None')
            prepared.append((im, np.concatenate([ch, np.zeros(4 - len(ch), np.int32)]), thr, bnd, m, p))
            spps = [3, 3, 3] + ([1] if m is not None else []) + ([3] if p is not None else [])
            tab, end = [], 0
            for spp in spps:                                   # as the call places them: every raster on a multiple of 256 bytes
                tab.append([end, H, W, spp, 0])
                end += (H * W * spp + 255) // 256 * 256
            need = self.lib.ecseg_tiff_encode_batch_bytes(_ptr(np.array(tab, np.int64)), len(tab))
            needs.append(need if need < 0 else need + end + 2 * H * W * im.shape[2] + 3 * 256)
        out = []
        for lo, hi in self._split_by_budget(needs, budget_bytes):
            chunk = prepared[lo:hi]
            n = len(chunk)
            shapes = np.array([[c[0].shape[0], c[0].shape[1], c[0].shape[2]] for c in chunk], np.int32)
            chans = np.ascontiguousarray(np.stack([c[1] for c in chunk]), np.int32)
            ptrs = lambda col: (C.c_void_p * n)(*[None if c[col] is None else c[col].ctypes.data for c in chunk])
            cap = 0
            for c in chunk:
                H, W = c[3].shape
                cap += 3 * self.lib.ecseg_tiff_encode_bound(H, W, 3) + (self.lib.ecseg_tiff_encode_bound(H, W, 1) if c[4] is not None else 0) + \
                    (self.lib.ecseg_tiff_encode_bound(H, W, 3) if c[5] is not None else 0)
            if cap < 0:
                raise ValueError('fish_render_tiff_many: an image that cannot be written as a TIFF')
            files = np.empty(max(cap, 1), np.uint8)
            ranges = np.zeros((n, 5, 2), np.int64)
            self._check(self.lib.ecseg_fish_render_tiff_batch(self.h, n, ptrs(0), _ptr(shapes), _ptr(chans), ptrs(2), ptrs(3), ptrs(4), ptrs(5),
                                                              _ptr(files), cap, _ptr(ranges)), 'ecseg_fish_render_tiff_batch')
            for i, c in enumerate(chunk):
                have = (True, True, True, c[4] is not None, c[5] is not None)
                out.append(tuple(files[o:o + k].tobytes() if h else None for (o, k), h in zip(ranges[i].tolist(), have)))
        return out

    # ---- stat_fish.batch: mask to file images of k images per call ------------------------------------------
    STAT_FISH_ITEM_KEYS = ('img', 'channels', 'mask', 'labels', 'weights', 'normal_threshold', 'intensity_thresholds', 'min_cc_size',
                           'mask_file', 'picture')

    @classmethod
    def _stat_fish_item(cls, item):
        """One item of ``stat_fish_many`` checked and made contiguous -> the tuple ``stat_fish_packed`` takes, or raises."""
        unknown = set(item) - set(cls.STAT_FISH_ITEM_KEYS)
        if unknown:
            raise ValueError('stat_fish_many: unknown item keys %s' % sorted(unknown))
        im = _u8(item['img'])
        if im.ndim != 3 or im.shape[2] not in (3, 4) or not im.size:
            raise ValueError('stat_fish_many takes non-empty (H, W, 3) or (H, W, 4) uint8 images')
        H, W, Cn = im.shape
        ch = np.ascontiguousarray(item['channels'], np.int32).reshape(-1)
        if len(ch) != Cn:
            raise ValueError('stat_fish_many takes one channel index per image channel (blue, green, red[, aqua])')
        mask, labels = item.get('mask'), item.get('labels')
        if (mask is None) == (labels is None):
            raise ValueError('stat_fish_many takes exactly one of mask and labels per image')
        if mask is not None:
            mask = _u8(mask)
            if mask.shape != (H, W):
                raise ValueError('stat_fish_many takes an (H, W) uint8 mask of the image\'s extent')
        else:
            labels = np.ascontiguousarray(labels)
            if labels.dtype != np.int32:
                if labels.dtype.kind not in 'iu' or (labels.size and (int(labels.max()) > 2 ** 31 - 1 or int(labels.min()) < -2 ** 31)):
                    raise ValueError('stat_fish_many takes integer labels that fit int32')
                labels = labels.astype(np.int32)
            if labels.shape != (H, W):
                raise ValueError('stat_fish_many takes an (H, W) label map of the image\'s extent')
        w = np.ascontiguousarray(item['weights'], np.float64)
        if w.ndim != 2 or w.shape[0] != w.shape[1] or not w.size:
            raise ValueError('stat_fish_many takes a square K x K kernel')
        ithr = np.ascontiguousarray(item['intensity_thresholds'], np.float64).reshape(-1)
        if len(ithr) != Cn - 1:
            raise ValueError('stat_fish_many takes one intensity threshold per probe channel (C - 1 of them)')
        mask_file, picture = item.get('mask_file'), item.get('picture')
        if mask_file is True:
            if mask is None:
                raise ValueError('stat_fish_many: mask_file=True needs a mask')
            mask_file = mask
        elif mask_file is not None:
            mask_file = _u8(mask_file)
        picture = None if picture is None else _u8(picture)
        if (mask_file is not None and mask_file.shape != (H, W)) or (picture is not None and picture.shape != (H, W, 3)):
            raise ValueError('stat_fish_many takes an (H, W) mask file raster and an (H, W, 3) picture of the image\'s extent, or None')
        return (im, np.concatenate([ch, np.zeros(4 - len(ch), np.int32)]), mask, labels, w, float(item['normal_threshold']),
                np.concatenate([ithr, np.zeros(3 - len(ithr))]), int(item['min_cc_size']), mask_file, picture)

    def _stat_fish_tables(self, chunk):
        shapes = np.array([c[0].shape for c in chunk], np.int32).reshape(-1, 3)
        ks = np.array([c[4].shape[0] for c in chunk], np.int32)
        flags = np.array([(c[3] is not None) | ((c[8] is not None) << 1) | ((c[8] is not None and c[8] is c[2]) << 2) | ((c[9] is not None) << 3)
                          for c in chunk], np.int32)
        return shapes, ks, flags

    def stat_fish_batch_bytes(self, chunk, record_capacity):
        """Device scratch one ``stat_fish_packed`` call over these prepared items needs (ecseg_stat_fish_batch_bytes; -1: refused)."""
        shapes, ks, flags = self._stat_fish_tables(chunk)
        return self.lib.ecseg_stat_fish_batch_bytes(len(chunk), _ptr(shapes), _ptr(ks), _ptr(flags), int(record_capacity))

    def stat_fish_packed(self, chunk, line_thickness, record_capacity, out_capacity=None, want_masks=False, poison=None):
        """ecseg_stat_fish_batch as it is over prepared items (``_stat_fish_item``) -> dict: ``n_cells`` (n,) int32, ``ranks`` int32 (the
        images' maps back to back), ``records`` int64 (record_capacity, 24), ``out`` uint8 with ``ranges`` (n, 5, 2), and with
        ``want_masks`` ``thresholded`` and ``boundaries`` (uint8, back to back).  ``out_capacity``: bytes of ``out`` (default: the sum of
        ecseg_tiff_encode_bound).  ``poison``: a byte every output buffer is filled with before the call (tests)."""
        n = len(chunk)
        shapes, ks, _ = self._stat_fish_tables(chunk)
        chans = np.ascontiguousarray(np.stack([c[1] for c in chunk]), np.int32) if n else np.zeros((0, 4), np.int32)
        ptrs = lambda col: (C.c_void_p * max(n, 1))(*[None if c[col] is None else c[col].ctypes.data for c in chunk])
        normal = np.array([c[5] for c in chunk], np.float64)
        ithr = np.ascontiguousarray(np.stack([c[6] for c in chunk]), np.float64) if n else np.zeros((0, 3))
        min_cc = np.array([c[7] for c in chunk], np.int32)
        px = [int(c[0].shape[0]) * int(c[0].shape[1]) for c in chunk]
        if out_capacity is None:
            out_capacity = 0
            for c in chunk:
                H, W = c[0].shape[:2]
                out_capacity += 3 * self.lib.ecseg_tiff_encode_bound(H, W, 3) + (self.lib.ecseg_tiff_encode_bound(H, W, 1) if c[8] is not None else 0) + \
                    (self.lib.ecseg_tiff_encode_bound(H, W, 3) if c[9] is not None else 0)
            if out_capacity < 0:
                raise ValueError('stat_fish_many: an image that cannot be written as a TIFF')
        cap = int(record_capacity)
        def new(shape, dt):
            a = np.empty(shape, dt)
            if poison is not None:
                a.view(np.uint8)[...] = poison
            return a
        res = dict(n_cells=new((max(n, 1),), np.int32), ranks=new((max(sum(px), 1),), np.int32), records=new((max(cap, 1), self.FISH_SPOT_INT64), np.int64),
                   out=new((max(int(out_capacity), 1),), np.uint8), ranges=new((max(n, 1), 5, 2), np.int64))
        if want_masks:
            res['thresholded'] = new((max(sum(p * (c[0].shape[2] - 1) for p, c in zip(px, chunk)), 1),), np.uint8)
            res['boundaries'] = new((max(sum(px), 1),), np.uint8)
        self._check(self.lib.ecseg_stat_fish_batch(self.h, n, ptrs(0), _ptr(shapes), _ptr(chans), ptrs(2), ptrs(3), _ptr(ks), ptrs(4), _ptr(normal),
                                                   _ptr(ithr), _ptr(min_cc), int(line_thickness), ptrs(8), ptrs(9), cap, _ptr(res['ranks']),
                                                   _ptr(res['records']), _ptr(res['n_cells']), _ptr(res['out']), int(out_capacity), _ptr(res['ranges']),
                                                   _ptr(res.get('thresholded')), _ptr(res.get('boundaries'))), 'ecseg_stat_fish_batch')
        res['n_cells'] = res['n_cells'][:n]
        res['ranges'] = res['ranges'][:n]
        return res

    def stat_fish_many(self, items, line_thickness, record_capacity=4096, budget_bytes=8 << 30, want_masks=False):
        """stat_fish from the mask to the file images for a list of images (ecseg_stat_fish_batch): per item what ``ccl_labels`` ->
        ``fish_spots`` -> ``fish_render_tiff_many`` give, in one device call per chunk.  An item is a dict: ``img`` (H, W, C) uint8,
        C = 3 or 4; ``channels`` its (blue, green, red[, aqua]) indices; exactly one of ``mask`` ((H, W) uint8, non-zero = nucleus,
        labelled 8-connected on the device) and ``labels`` ((H, W) integer map, used as given); ``weights`` (K x K float64),
        ``normal_threshold``, ``intensity_thresholds`` (C - 1), ``min_cc_size``; optional ``mask_file`` (an (H, W) uint8 raster, or True
        for the mask itself) and ``picture`` ((H, W, 3) uint8), encoded beside the three colour files.
        -> per item ``(ranks, records, files)``: the (H, W) int32 dense ranks (0 background, 1 .. n in ascending label order), the
        (n, 24) int64 records of ``fish_spots`` and the tuple (original, with_segmentation, lsq, mask file or None, picture or None) of
        ``bytes``; with ``want_masks`` a fourth and fifth entry, ``fish_spots``' thresholded and boundaries.  An item that fails
        validation has its exception in its place and takes no part; the others are unaffected.  ``record_capacity`` is grown and the
        call repeated once when the chunk holds more cells.  The list goes in one call while ecseg_stat_fish_batch_bytes stays within
        ``budget_bytes``, else in consecutive calls (an item above the budget alone goes alone); the returned list is the same."""
        out = [None] * len(items)
        good = []
        for k, item in enumerate(items):
            try:
                good.append((k, self._stat_fish_item(item)))
            except (ValueError, TypeError, KeyError) as e:
                out[k] = e
        needs = [self.stat_fish_batch_bytes([c], 0) for _, c in good]
        for lo, hi in self._split_by_budget(needs, budget_bytes):
            chunk = [c for _, c in good[lo:hi]]
            res = self.stat_fish_packed(chunk, line_thickness, record_capacity, want_masks=want_masks)
            total = int(res['n_cells'].sum())
            if total > record_capacity:                      # the counts alone came back: once more with room for them
                res = self.stat_fish_packed(chunk, line_thickness, total, want_masks=want_masks)
            p0 = r0 = t0 = 0
            for (k, _), c, n, rng in zip(good[lo:hi], chunk, res['n_cells'].tolist(), res['ranges'].tolist()):
                H, W, Cn = c[0].shape
                have = (True, True, True, c[8] is not None, c[9] is not None)
                files = tuple(res['out'][o:o + m].tobytes() if hv else None for (o, m), hv in zip(rng, have))
                entry = (res['ranks'][p0:p0 + H * W].reshape(H, W).copy(), res['records'][r0:r0 + n].copy(), files)
                if want_masks:
                    entry += (res['thresholded'][t0:t0 + H * W * (Cn - 1)].reshape(H, W, Cn - 1).copy(), res['boundaries'][p0:p0 + H * W].reshape(H, W).copy())
                out[k] = entry
                p0 += H * W; r0 += n; t0 += H * W * (Cn - 1)
        return out

    # ---- min-cut splitter -------------------------------------------------------------------------------
    MIN_CUT_MAX_DIST = 32         # ECSEG_MIN_CUT_MAX_DIST
    MIN_CUT_LDS_PIXELS = 10240     # ECSEG_MIN_CUT_LDS_PIXELS

    def min_cut(self, tasks, dist):
        """A batch of max-flow tasks (ecseg_min_cut; the network is in include/ecseg_hip.h).  ``tasks``: a sequence of
        (window, source, sink) with window a 2-D uint8 / bool array, non-zero = pixel, and source / sink (row, column) pixels of
        it -> (list of uint8 windows, 1 = on the source's side of the minimal minimum cut, int32 array of the max-flow values)."""
        wins = [_u8(t[0]) for t in tasks]
        if any(w.ndim != 2 for w in wins):
            raise ValueError('min_cut takes 2-D windows')
        desc = np.zeros((len(wins), 8), np.int32)
        offs = np.concatenate([[0], np.cumsum([w.size for w in wins], dtype=np.int64)]).astype(np.int64)
        if offs[-1] >= 2 ** 31:
            raise ValueError('min_cut: the windows of one call must stay below 2^31 bytes')
        for k, (w, t) in enumerate(zip(wins, tasks)):
            desc[k, :7] = (offs[k], w.shape[0], w.shape[1], int(t[1][0]), int(t[1][1]), int(t[2][0]), int(t[2][1]))
        packed = np.concatenate([w.reshape(-1) for w in wins]) if wins else np.zeros(0, np.uint8)
        side = np.zeros(packed.size, np.uint8)
        flow = np.zeros(len(wins), np.int32)
        self._check(self.lib.ecseg_min_cut(self.h, _ptr(packed), packed.size, _ptr(desc), len(wins), int(dist), _ptr(side), _ptr(flow)),
                    'ecseg_min_cut')
        return [side[offs[k]:offs[k + 1]].reshape(w.shape) for k, w in enumerate(wins)], flow

    def min_cut_regions_raw(self, mask, coeff, min_rad, region_capacity, center_capacity, window_capacity):
        """One ecseg_min_cut_regions call with the given capacities -> (labels, (n_cells, n_regions, n_centers, window_pixels),
        regions, centers, windows, comp): the four buffers as allocated, preset to -1 / 255, untouched when a capacity is short."""
        m = _u8(mask)
        if m.ndim != 2:
            raise ValueError('min_cut_regions takes a 2-D mask')
        H, W = m.shape
        labels = np.empty((H, W), np.int32)
        regions = np.full((int(region_capacity), 8), -1, np.int32)
        centers = np.full((int(center_capacity), 8), -1, np.int32)
        windows = np.full(int(window_capacity), 255, np.uint8)
        comp = np.full(int(window_capacity), -1, np.int32)
        counts = np.zeros(3, np.int32)
        wpx = C.c_longlong(0)
        self._check(self.lib.ecseg_min_cut_regions(self.h, _ptr(m), H, W, float(coeff), int(min_rad), regions.shape[0], centers.shape[0],
                                                   windows.size, _ptr(labels), _ptr(counts[0:]), _ptr(regions), _ptr(counts[1:]), _ptr(centers),
                                                   _ptr(counts[2:]), _ptr(windows), _ptr(comp), C.byref(wpx)), 'ecseg_min_cut_regions')
        return labels, (int(counts[0]), int(counts[1]), int(counts[2]), int(wpx.value)), regions, centers, windows, comp

    def min_cut_regions(self, mask, coeff, min_rad=10):
        """What binary_seg_to_instance_min_cut needs before its first max-flow, in one device call (ecseg_min_cut_regions; the records
        are in include/ecseg_hip.h) -> (labels (H, W) int32, regions (n, 8) int32, centers (m, 8) int32, windows, comp): ``windows``
        and ``comp`` hold one (h, w) array per region.  The capacities are guessed and grown by one repeat call."""
        m = _u8(mask)
        caps = getattr(self, '_mcr_caps', (64, 256, 1 << 18))
        got = self.min_cut_regions_raw(m, coeff, min_rad, *caps)
        _, n_reg, n_cen, wpx = got[1]
        if n_reg > caps[0] or n_cen > caps[1] or wpx > caps[2]:
            caps = (max(caps[0], n_reg), max(caps[1], n_cen), max(caps[2], wpx))
            got = self.min_cut_regions_raw(m, coeff, min_rad, *caps)
        self._mcr_caps = caps                                # the next image of a folder is alike: one call then
        labels, _, regions, centers, windows, comp = got
        regions, centers = regions[:n_reg], centers[:n_cen]
        wins = [windows[r[5]:r[5] + r[3] * r[4]].reshape(r[3], r[4]) for r in regions]
        comps = [comp[r[5]:r[5] + r[3] * r[4]].reshape(r[3], r[4]) for r in regions]
        return labels, regions, centers, wins, comps

    # ---- NuSeT's network stage ---------------------------------------------------------------------------
    RPN_MAX_CANDIDATES = 1 << 22   # ECSEG_RPN_MAX_CANDIDATES
    RPN_MAX_PRE_NMS = 8192         # ECSEG_RPN_MAX_PRE_NMS

    def nuset_forward(self, x, cls_tensor, bbox_tensor):
        """(H, W) float32 normalised image -> uint8 (H, W) argmax mask of the loaded plan's 2-channel logits (ecseg_nuset_forward).
        ``cls_tensor`` / ``bbox_tensor``: the plan's RPN tensors (``plan.layer_tensor``), which stay on the handle for
        ``rpn_proposals_last``."""
        if self.plan is None:
            raise EcsegError('no model loaded')
        a = np.ascontiguousarray(x, np.float32)
        if a.ndim != 2:
            raise ValueError('nuset_forward takes one (H, W) image')
        mask = np.empty(a.shape, np.uint8)
        self._check(self.lib.ecseg_nuset_forward(self.h, _ptr(a), a.shape[0], a.shape[1], int(cls_tensor), int(bbox_tensor), _ptr(mask)),
                    'ecseg_nuset_forward')
        return mask

    @staticmethod
    def _rpn_args(ref_anchors, pre_nms_top_n, post_nms_top_n):
        ref = np.ascontiguousarray(ref_anchors, np.float64)
        if ref.ndim != 2 or ref.shape[1] != 4:
            raise ValueError('ref_anchors must be (A, 4) float64')
        cap = max(min(int(post_nms_top_n), int(pre_nms_top_n)), 1)
        return ref, np.empty(cap, np.float32), np.empty((cap, 4), np.float32), np.empty(cap, np.int32)

    def rpn_proposals(self, cls_score, bbox_pred, ref_anchors, stride, im_h, im_w, nms_threshold, pre_nms_top_n=6000, post_nms_top_n=800):
        """RPNProposal on host tensors (ecseg_rpn_proposals; the arithmetic is in include/ecseg_hip.h): ``cls_score`` (fh, fw, 2A) and
        ``bbox_pred`` (fh, fw, 4A) float32, ``ref_anchors`` (A, 4) float64 -> (scores float32 (n,) descending, proposals float32 (n, 4)
        as (x1, y1, x2, y2), int32 (n,) flat indices (y * fw + x) * A + a of the selected candidates)."""
        ref, sc, pr, ix = self._rpn_args(ref_anchors, pre_nms_top_n, post_nms_top_n)
        c = np.ascontiguousarray(cls_score, np.float32)
        b = np.ascontiguousarray(bbox_pred, np.float32)
        A = ref.shape[0]
        if c.ndim != 3 or b.ndim != 3 or c.shape[2] != 2 * A or b.shape != c.shape[:2] + (4 * A,):
            raise ValueError('rpn_proposals takes (fh, fw, 2A) scores and (fh, fw, 4A) deltas for (A, 4) reference anchors')
        n = C.c_int32()
        self._check(self.lib.ecseg_rpn_proposals(self.h, _ptr(c), _ptr(b), c.shape[0], c.shape[1], A, _ptr(ref), int(stride), int(im_h), int(im_w),
                                                 float(nms_threshold), int(pre_nms_top_n), int(post_nms_top_n), C.byref(n), _ptr(sc), _ptr(pr),
                                                 _ptr(ix)), 'ecseg_rpn_proposals')
        return sc[:n.value], pr[:n.value], ix[:n.value]

    def rpn_proposals_last(self, ref_anchors, stride, im_h, im_w, nms_threshold, pre_nms_top_n=6000, post_nms_top_n=800):
        """The same on the RPN tensors the last ``nuset_forward`` left on the device (ecseg_rpn_proposals_last)."""
        ref, sc, pr, ix = self._rpn_args(ref_anchors, pre_nms_top_n, post_nms_top_n)
        n = C.c_int32()
        self._check(self.lib.ecseg_rpn_proposals_last(self.h, ref.shape[0], _ptr(ref), int(stride), int(im_h), int(im_w), float(nms_threshold),
                                                      int(pre_nms_top_n), int(post_nms_top_n), C.byref(n), _ptr(sc), _ptr(pr), _ptr(ix)),
                    'ecseg_rpn_proposals_last')
        return sc[:n.value], pr[:n.value], ix[:n.value]

    @staticmethod
    def _mask_u8(mask, what):
        m = np.asarray(mask)
        if m.ndim != 2:
            raise ValueError('%s takes one (H, W) mask' % what)
        if m.dtype.kind not in 'biu':
            raise TypeError('%s: expected a bool / integer mask, got %s' % (what, m.dtype))
        return np.ascontiguousarray(m != 0, np.uint8) if m.dtype != np.uint8 else np.ascontiguousarray(m)

    def marker_watershed(self, mask, rows, cols, labels):
        """(H, W) bool / integer mask + the ordered marker list (``nuset.watershed_markers``) -> uint8 (H, W): the mask where the
        marker watershed with lines put a label, 0 on the lines and where no marker reaches (ecseg_marker_watershed)."""
        m = self._mask_u8(mask, 'marker_watershed')
        r, c, l = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (rows, cols, labels))
        if not (len(r) == len(c) == len(l)):
            raise ValueError('marker_watershed: rows, cols and labels differ in length')
        out = np.empty(m.shape, np.uint8)
        self._check(self.lib.ecseg_marker_watershed(self.h, _ptr(m), m.shape[0], m.shape[1], _ptr(r), _ptr(c), _ptr(l), len(r), _ptr(out)),
                    'ecseg_marker_watershed')
        return out

    def marker_watershed_stages(self, mask, rows, cols, labels):
        """Test-only (ecseg_marker_watershed_stages_debug): ``marker_watershed`` with what its stages left on the device ->
        dict(rw int32, filled uint8, d2 int32, lab int32, out uint8), each (H, W).  ``rw`` and ``d2`` are 0 off the mask."""
        m = self._mask_u8(mask, 'marker_watershed_stages')
        r, c, l = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (rows, cols, labels))
        if not (len(r) == len(c) == len(l)):
            raise ValueError('marker_watershed_stages: rows, cols and labels differ in length')
        res = dict(rw=np.empty(m.shape, np.int32), filled=np.empty(m.shape, np.uint8), d2=np.empty(m.shape, np.int32),
                   lab=np.empty(m.shape, np.int32), out=np.empty(m.shape, np.uint8))
        self._check(self.lib.ecseg_marker_watershed_stages_debug(self.h, _ptr(m), m.shape[0], m.shape[1], _ptr(r), _ptr(c), _ptr(l), len(r),
                                                                 _ptr(res['out']), _ptr(res['rw']), _ptr(res['filled']), _ptr(res['d2']),
                                                                 _ptr(res['lab'])), 'ecseg_marker_watershed_stages_debug')
        return res

    WATERSHED_BATCH_MAX_IMAGES = 1024     # ECSEG_WATERSHED_BATCH_MAX_IMAGES

    def marker_watershed_batch_stages(self, masks, images, rows, cols, labels):
        """Test-only (ecseg_marker_watershed_batch_stages_debug): ``marker_watershed_packed`` with the stage products -> one dict per
        image as ``marker_watershed_stages`` returns it, cut out of the packed buffers at the image's offset."""
        buf = np.ascontiguousarray(masks, np.uint8).reshape(-1)
        tab = np.ascontiguousarray(images, np.int64).reshape(-1, 5)
        r, c, l = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (rows, cols, labels))
        if not (len(r) == len(c) == len(l)):
            raise ValueError('marker_watershed_batch_stages: rows, cols and labels differ in length')
        res = dict(rw=np.zeros(buf.size, np.int32), filled=np.zeros(buf.size, np.uint8), d2=np.zeros(buf.size, np.int32),
                   lab=np.zeros(buf.size, np.int32), out=np.zeros(buf.size, np.uint8))
        self._check(self.lib.ecseg_marker_watershed_batch_stages_debug(self.h, _ptr(buf), buf.size, _ptr(tab), len(tab), _ptr(r), _ptr(c), _ptr(l),
                                                                       len(r), _ptr(res['out']), _ptr(res['rw']), _ptr(res['filled']),
                                                                       _ptr(res['d2']), _ptr(res['lab'])),
                    'ecseg_marker_watershed_batch_stages_debug')
        return [{k: v[o:o + H * W].reshape(H, W).copy() for k, v in res.items()} for o, H, W, _, _ in tab.tolist()]

    def marker_watershed_packed(self, masks, images, rows, cols, labels):
        """ecseg_marker_watershed_batch as it is: ``masks`` a 1-D uint8 buffer, ``images`` (n, 5) int64 rows (byte offset, H, W, first
        marker, markers), the three int32 marker lists of all images -> the uint8 buffer of the results, laid out as ``masks`` and 0
        outside every image."""
        buf = np.ascontiguousarray(masks, np.uint8).reshape(-1)
        tab = np.ascontiguousarray(images, np.int64).reshape(-1, 5)
        r, c, l = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (rows, cols, labels))
        if not (len(r) == len(c) == len(l)):
            raise ValueError('marker_watershed_packed: rows, cols and labels differ in length')
        out = np.empty(buf.size, np.uint8)
        self._check(self.lib.ecseg_marker_watershed_batch(self.h, _ptr(buf), buf.size, _ptr(tab), len(tab), _ptr(r), _ptr(c), _ptr(l), len(r),
                                                          _ptr(out)), 'ecseg_marker_watershed_batch')
        return out

    def marker_watershed_batch(self, masks, markers, budget_bytes=8 << 30):
        """``marker_watershed`` over a list of images at once (ecseg_marker_watershed_batch: one flood wave per image, side by side).
        ``masks``: a list of (H, W) bool / integer masks of any extents; ``markers``: per mask its ``(rows, cols, labels)``, or None
        for "leave the mask as it is" (what ``nuset.watershed_markers`` returns for its two early branches): such an image does not go
        to the device and comes back as given.  -> the list of uint8 (H, W) results, each the bytes ``marker_watershed`` gives that image
        alone.  The images are packed back to back and go in one call while ecseg_marker_watershed_batch_bytes stays within
        ``budget_bytes`` of device scratch (and WATERSHED_BATCH_MAX_IMAGES images), else in several calls over consecutive images;
        an image that exceeds the budget alone goes alone."""
        if len(masks) != len(markers):
            raise ValueError('marker_watershed_batch takes one marker entry (or None) per mask')
        out = [None] * len(masks)
        todo = []                                              # (position, mask, rows, cols, labels, foreground pixels)
        for k, (mask, mk) in enumerate(zip(masks, markers)):
            if mk is None:
                out[k] = mask
                continue
            m = self._mask_u8(mask, 'marker_watershed_batch')
            r, c, l = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in mk)
            if not (len(r) == len(c) == len(l)):
                raise ValueError('marker_watershed_batch: rows, cols and labels of image %d differ in length' % k)
            todo.append((k, m, r, c, l, int(np.count_nonzero(m))))

        def table(chunk):
            tab, off, first = np.zeros((len(chunk), 5), np.int64), 0, 0
            for j, (_, m, r, _, _, _) in enumerate(chunk):
                tab[j] = (off, m.shape[0], m.shape[1], first, len(r))
                off += m.size
                first += len(r)
            return tab

        def need(chunk):
            tab = table(chunk)
            fg = np.array([e[5] for e in chunk], np.int64)
            return self.lib.ecseg_marker_watershed_batch_bytes(_ptr(tab), len(tab), _ptr(fg))

        chunks, cur = [], []
        for entry in todo:
            if cur and (len(cur) >= self.WATERSHED_BATCH_MAX_IMAGES or not 0 <= need(cur + [entry]) <= budget_bytes):
                chunks.append(cur)
                cur = []
            cur.append(entry)
        if cur:
            chunks.append(cur)
        for chunk in chunks:
            tab = table(chunk)
            cat = lambda arrs, dt: np.concatenate([a.reshape(-1) for a in arrs]) if arrs else np.zeros(0, dt)
            res = self.marker_watershed_packed(cat([e[1] for e in chunk], np.uint8), tab, cat([e[2] for e in chunk], np.int32),
                                               cat([e[3] for e in chunk], np.int32), cat([e[4] for e in chunk], np.int32))
            for (k, m, _, _, _, _), row in zip(chunk, tab):
                out[k] = res[row[0]:row[0] + m.size].reshape(m.shape)
        return out

    def clean_nuclei(self, mask, nuclei_size_T, want_cleaned=False):
        """(H, W) bool / integer mask, != 0 foreground (``_watershed``'s output) -> (uint8 0 / 255 final mask, mean_area) (ecseg_clean_nuclei:
        ``clean_image`` and the threshold of src/utils.py:159-162); ``want_cleaned``: ``clean_image``'s own 0 / 1 output as a third
        value."""
        m = self._mask_u8(mask, 'clean_nuclei')
        out = np.empty(m.shape, np.uint8)
        cleaned = np.empty(m.shape, np.uint8) if want_cleaned else None
        mean = C.c_double()
        self._check(self.lib.ecseg_clean_nuclei(self.h, _ptr(m), m.shape[0], m.shape[1], int(nuclei_size_T), _ptr(out), _ptr(cleaned),
                                                C.byref(mean)), 'ecseg_clean_nuclei')
        return (out, mean.value, cleaned) if want_cleaned else (out, mean.value)

    @staticmethod
    def _rescale_u8(a, what):
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError('%s takes one (H, W) image' % what)
        if a.dtype != np.uint8:
            raise ValueError('%s: expected uint8, got %s (scikit-image 0.18 filters in the input\'s dtype: another dtype is another '
                             'result)' % (what, a.dtype))
        return np.ascontiguousarray(a)

    def rescale_down(self, image_u8, scale):
        """``rescale(image, scale, anti_aliasing=True)`` of scikit-image 0.18 (src/utils.py:136) on a uint8 (H, W) image, 0 < scale <= 1 ->
        (float64 (out_h, out_w) in [0, 1], the Gaussian-filtered uint8 (H, W) image) (ecseg_rescale_down; the extent and the weights
        are computed here in float64: ``rescale_extent``, ``rescale_weights``)."""
        a = self._rescale_u8(image_u8, 'rescale_down')
        H, W = a.shape
        oh, ow = rescale_extent(a.shape, scale)
        wy, wx = rescale_weights(H, max(oh, 1)), rescale_weights(W, max(ow, 1))
        out = np.empty((max(oh, 0), max(ow, 0)), np.float64)
        filtered = np.empty((H, W), np.uint8)
        self._check(self.lib.ecseg_rescale_down(self.h, _ptr(a), H, W, oh, ow, _ptr(wy), len(wy) // 2, _ptr(wx), len(wx) // 2, _ptr(filtered),
                                                _ptr(out)), 'ecseg_rescale_down')
        return out, filtered

    def rescale_mask_up(self, cleaned, scale, nuclei_size_T):
        """``rescale(cleaned, scale)`` (``scale`` = 1 / scale_ratio >= 1, as the caller computes it) of ``clean_image``'s uint8 0 / 1
        output, the min-max scaling, the threshold and ``remove_small_objects(bool, nuclei_size_T)`` of src/utils.py:157-162 -> uint8
        0 / 255 of extent ``np.round(scale * shape)`` (ecseg_rescale_mask_up)."""
        c = self._rescale_u8(cleaned, 'rescale_mask_up')
        oh, ow = rescale_extent(c.shape, scale)
        out = np.empty((max(oh, 0), max(ow, 0)), np.uint8)
        self._check(self.lib.ecseg_rescale_mask_up(self.h, _ptr(c), c.shape[0], c.shape[1], oh, ow, int(nuclei_size_T), _ptr(out)),
                    'ecseg_rescale_mask_up')
        return out

    # ---- timing ---------------------------------------------------------------------------------------
    def timings(self):
        t = np.zeros(5, np.float32)
        self._check(self.lib.ecseg_get_timings(self.h, _ptr(t)), 'ecseg_get_timings')
        return dict(zip(self.T_NAMES, [float(v) for v in t]))

    def set_kernel_profiling(self, on):
        self._check(self.lib.ecseg_set_kernel_profiling(self.h, int(bool(on))), 'ecseg_set_kernel_profiling')

    def conv_profile(self):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._check(self.lib.ecseg_get_conv_profile(self.h, C.byref(ms), C.byref(n), C.byref(fl)), 'ecseg_get_conv_profile')
        return ms.value, n.value, fl.value

    def conv_launch_profile(self, max_records=4096):
        """Per-launch records of the last profiled call: list of dicts (op, kind, ms, flops, executed_flops)."""
        op = np.zeros(max_records, np.int32); kind = np.zeros(max_records, np.int32)
        ms = np.zeros(max_records, np.float32); fl = np.zeros(max_records, np.float64); ex = np.zeros(max_records, np.float64)
        n = self.lib.ecseg_get_conv_launch_profile(self.h, max_records, _ptr(op), _ptr(kind), _ptr(ms), _ptr(fl), _ptr(ex))
        if n < 0:
            self._check(n, 'ecseg_get_conv_launch_profile')
        return [dict(op=int(op[k]), kind=int(kind[k]), ms=float(ms[k]), flops=float(fl[k]), executed_flops=float(ex[k]))
                for k in range(n)]

    def debug_peek(self, n=32):
        out = np.zeros(n, np.float32)
        self._check(self.lib.ecseg_debug_peek(self.h, _ptr(out), n), 'ecseg_debug_peek')
        return out

    def conv_executed_flops(self):
        fl = C.c_double()
        self._check(self.lib.ecseg_get_conv_executed_flops(self.h, C.byref(fl)), 'ecseg_get_conv_executed_flops')
        return fl.value


class Comm:
    """RCCL communicator of the C ABI (csrc/comm.hip): the record all-gather without torch.distributed.  Rank 0 creates the
    id with ``Comm.unique_id()`` and hands the 128 bytes to the other ranks; then every rank constructs its ``Comm``."""

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.ecseg_comm_unique_id(buf, 128)
        if rc != 0:
            e = EcsegError('ecseg_comm_unique_id failed (%d): %s' % (rc, lib.ecseg_comm_last_error().decode()))
            e.code = rc
            raise e
        return buf.raw

    def __init__(self, unique_id, rank, world, device):
        self.lib = load_library()
        c = C.c_void_p()
        rc = self.lib.ecseg_comm_create(C.byref(c), C.c_char_p(bytes(unique_id)), int(rank), int(world), int(device))
        if rc != 0:
            e = EcsegError('ecseg_comm_create(rank %d of %d, device %d) failed (%d): %s'
                           % (rank, world, device, rc, self.lib.ecseg_comm_last_error().decode()))
            e.code = rc
            raise e
        self.c, self.rank, self.world = c, int(rank), int(world)

    def _check(self, rc, what):
        if rc != 0:
            e = EcsegError('%s failed (%d): %s' % (what, rc, self.lib.ecseg_comm_last_error().decode()))
            e.code = rc
            raise e

    def allgather_records(self, rec):
        """rec: int64 (padded_len, 16) host array -> (world * padded_len, 16), rank-major."""
        a = np.ascontiguousarray(rec, np.int64)
        out = np.empty((self.world * a.shape[0], a.shape[1]), np.int64)
        self._check(self.lib.ecseg_allgather_records(self.c, _ptr(a), a.shape[0], _ptr(out)), 'ecseg_allgather_records')
        return out

    def allgather_records_dev(self, send_ptr, n_records, recv_ptr, stream=None):
        self._check(self.lib.ecseg_allgather_records_dev(self.c, C.c_void_p(send_ptr), int(n_records), C.c_void_p(recv_ptr),
                                                         C.c_void_p(stream) if stream else None), 'ecseg_allgather_records_dev')

    def close(self):
        if getattr(self, 'c', None):
            self.lib.ecseg_comm_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
