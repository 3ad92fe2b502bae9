"""Which rows of tests/test_gpu_scratch.py run each ``lay_out`` call site of the drivers' scratch arenas (csrc/ctx.h).  Not a test
module: tests/test_gpu_scratch.py holds a driver per row named here, tests/test_scratch_rows.py holds the call sites of
ecseg_amd/csrc to this table.  A site is (the function it stands in, the arena, the layouts it places); a layout is named by its
layout function (``*_bufs``, ``post_workspace``), a buffer taken bare in the lambda (``c.take<T>(...)``) by ``take@<function>``.
A new driver has a new site even where it reuses a layout function, so it needs a row here.  Sites in helpers (ensure_post,
open_dense_cells, the *_driver bodies of drivers_nuset.hip) are keyed by the helper: their rows are the entries that reach them."""

ROWS = (
    # the nine of the first scratch test
    'nuclei_regions', 'fish_distances', 'fish_spots', 'min_cut', 'rpn_proposals', 'clean_nuclei', 'marker_watershed', 'rescale_down',
    'rescale_mask_up',
    # every arena driver added since
    'classify_nucleus_crops', 'iseg_classifier_inputs', 'interseg_batch', 'stat_fish_batch', 'min_cut_regions', 'marker_watershed_batch',
    'nuset_forward', 'fish_render', 'fish_render_tiff', 'fish_render_tiff_batch', 'tiff_encode', 'tiff_encode_batch', 'tiff_decode',
    'tiff_decode_batch', 'png_labels_encode', 'png_channel_encode', 'overlay_files', 'ccl_pass', 'post_workspace', 'meta_segment_files',
    'meta_segment_tiffs',
)

SITE_ROWS = {
    # drivers_interseg.hip
    ('ecseg_nuclei_regions', 'keep_arena', ('region_map_bufs',)): ('nuclei_regions', 'classify_nucleus_crops'),     # iseg
    ('ecseg_nuclei_regions', 'call_arena', ('region_bufs',)): ('nuclei_regions', 'classify_nucleus_crops'),
    ('ecseg_nucleus_crops', 'call_arena', ('crop_bufs',)): ('nuclei_regions',),                                     # (the row runs nucleus_crops on its map)
    ('ecseg_classify_nucleus_crops', 'call_arena', ('classify_bufs',)): ('classify_nucleus_crops',),
    ('ecseg_iseg_classifier_inputs_debug', 'call_arena', ('classify_bufs', 'take@ecseg_iseg_classifier_inputs_debug')): ('iseg_classifier_inputs',),
    ('ecseg_interseg_batch', 'call_arena', ('iseg_batch_bufs',)): ('interseg_batch',),
    # segment.hip
    ('ensure_post', 'post_arena', ('post_workspace',)): ('post_workspace', 'nuclei_regions', 'interseg_batch', 'stat_fish_batch', 'min_cut_regions',
                                                         'ccl_pass', 'overlay_files', 'meta_segment_files', 'meta_segment_tiffs'),
    ('meta_segment_run', 'call_arena', ('tiff_encode_bufs', 'png_encode_bufs', 'tiff_decode_batch_bufs')): ('meta_segment_files', 'meta_segment_tiffs'),
    ('meta_segment_run', 'pre_arena', ('tiff_decode_batch_bufs',)): ('meta_segment_tiffs',),                        # the decode-ahead
    # drivers_fish.hip
    ('open_dense_cells', 'call_arena', ('cell_index_bufs',)): ('fish_distances', 'fish_spots'),
    ('ecseg_fish_distances', 'count_arena', ('fishdist_bufs',)): ('fish_distances',),
    ('ecseg_fish_spots', 'count_arena', ('fishspot_bufs',)): ('fish_spots',),
    ('ecseg_fish_render', 'call_arena', ('fish_render_bufs',)): ('fish_render',),
    ('ecseg_fish_render_tiff', 'call_arena', ('fish_render_bufs', 'tiff_encode_bufs')): ('fish_render_tiff',),
    ('ecseg_fish_render_tiff_batch', 'call_arena', ('tiff_encode_batch_bufs', 'take@ecseg_fish_render_tiff_batch')): ('fish_render_tiff_batch',),
    ('ecseg_stat_fish_batch', 'call_arena', ('fs_batch_bufs', 'tiff_encode_batch_bufs')): ('stat_fish_batch',),
    ('ecseg_stat_fish_batch', 'count_arena', ('fs_batch_cell_bufs',)): ('stat_fish_batch',),
    ('ecseg_min_cut', 'call_arena', ('mincut_bufs',)): ('min_cut',),
    ('ecseg_min_cut_regions', 'call_arena', ('mcr_open_bufs',)): ('min_cut_regions',),
    ('ecseg_min_cut_regions', 'count_arena', ('take@ecseg_min_cut_regions',)): ('min_cut_regions',),
    ('ecseg_min_cut_regions', 'count_arena', ('mcr_region_bufs',)): ('min_cut_regions',),
    # drivers_nuset.hip
    ('rpn_driver', 'call_arena', ('rpn_bufs',)): ('rpn_proposals', 'nuset_forward'),                                 # (nuset_forward's row ends in rpn_proposals_last)
    ('marker_watershed_driver', 'call_arena', ('watershed_bufs',)): ('marker_watershed',),
    ('marker_watershed_batch_driver', 'call_arena', ('watershed_batch_bufs',)): ('marker_watershed_batch',),
    ('ecseg_nuset_forward', 'call_arena', ('nuset_mask_bufs',)): ('nuset_forward',),
    ('ecseg_clean_nuclei', 'call_arena', ('clean_bufs',)): ('clean_nuclei',),
    ('ecseg_rescale_down', 'call_arena', ('rescale_down_bufs',)): ('rescale_down',),
    ('ecseg_rescale_mask_up', 'call_arena', ('rescale_up_bufs',)): ('rescale_mask_up',),
    # drivers_post.hip
    ('ecseg_ccl_pass_debug', 'call_arena', ('ccl_pass_export_bufs',)): ('ccl_pass',),
    ('ecseg_overlay_files', 'call_arena', ('gray_encode_bufs', 'take@ecseg_overlay_files')): ('overlay_files',),
    # drivers_files.hip
    ('ecseg_tiff_encode', 'call_arena', ('tiff_encode_bufs',)): ('tiff_encode',),
    ('ecseg_tiff_encode_batch', 'call_arena', ('tiff_encode_batch_bufs',)): ('tiff_encode_batch',),
    ('ecseg_tiff_decode', 'call_arena', ('tiff_decode_batch_bufs',)): ('tiff_decode',),
    ('ecseg_tiff_decode_batch', 'call_arena', ('tiff_decode_batch_bufs',)): ('tiff_decode_batch',),
    ('ecseg_png_labels_encode', 'call_arena', ('png_encode_bufs',)): ('png_labels_encode',),
    ('ecseg_png_channel_encode', 'call_arena', ('gray_encode_bufs',)): ('png_channel_encode',),
}

# site -> why no row runs it
EXEMPT = {}
