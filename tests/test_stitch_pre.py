"""The two ends of the post-processing without a GPU: tests/stitch_pre_ref.py (what tests/test_gpu_stitch_pre.py holds
csrc/stitch_preprocess_kernels.hip to) against ``oracle.tiling``, ``oracle.quant`` and ``oracle.preprocess`` on every case of
tests/stitch_pre_cases.py and against the committed stitch maps; the cases against what their names promise; the CONDITION that makes
the histogram set worth running - on at least 100 of its histograms Otsu with its two products contracted into fused multiply-adds
(``otsu_fused``) inverts where plain float64 does not, or the other way round; and the MUTANTS, each a slip a kernel could make, with
the case that catches it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stitch_pre_cases as cases             # noqa: E402
import stitch_pre_ref as ref                 # noqa: E402

from ecseg_amd import _lib                   # noqa: E402
from oracle import preprocess as o_pre       # noqa: E402
from oracle import quant as o_quant          # noqa: E402
from oracle import tiling as o_tiling        # noqa: E402

PRE_CASES = cases.preprocess_cases()
PRE_NAMES = [c['name'] for c in PRE_CASES]


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(HERE, '..', 'include', 'ecseg_hip.h')).read()
    assert 'still 5 - additive: ecseg_stitch_stages_debug' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    for name, method in (('ecseg_stitch_stages_debug', 'stitch_stages'), ('ecseg_preprocess_stages_debug', 'preprocess_stages'),
                         ('ecseg_otsu_debug', 'otsu')):
        assert name in _lib.EXPORTS and name in hdr and hasattr(_lib.Handle, method)


# ---- the restatement against the oracle and the committed maps --------------------------------------------------------------------
def test_stitch_maps_equal_the_committed_maps(golden_dir):
    g = np.load(os.path.join(golden_dir, 'tiling.npz'), allow_pickle=False)
    assert len(g['sizes']) == 8
    for H, W in g['sizes'].tolist():
        key = '%dx%d' % (H, W)
        assert np.array_equal(ref.positions(H, W), g['pos_' + key]), key
        m = ref.stitch_map(H, W)
        w = m >= 0
        assert np.array_equal(np.where(w, m >> 16, -1), g['src_patch_' + key]), key
        assert np.array_equal(((m >> 8) & 255)[w], g['src_y_' + key][w]) and np.array_equal((m & 255)[w], g['src_x_' + key][w]), key


def _oracle_stitch(c):
    """labels, tie-risk counts and stitched probabilities of a stitch case from oracle.tiling and oracle.quant, image by image."""
    H, W, n = c['H'], c['W'], c['n_img']
    pos = o_tiling.patch_positions(H, W)
    written = o_tiling.stitch_source_map(pos)[0] >= 0
    labels, ties, probs = [], [], []
    for k in range(n):
        canvas = o_tiling.stitch(c['probs'][k * len(pos):(k + 1) * len(pos), :, :, :4], pos)
        q = o_quant.quantise_u8(canvas).astype(np.int64)
        top2 = np.sort(q, axis=-1)[..., -2:]
        labels.append(o_quant.argmax_first(q))
        ties.append(int((written & (top2[..., 1] - top2[..., 0] <= 1)).sum()))
        probs.append(canvas)
    return np.stack(labels), np.array(ties), np.stack(probs)


def _check_stitch_against_the_oracle(c):
    got = ref.stitch(c['probs'], c['n_img'], c['H'], c['W'])
    labels, ties, probs = _oracle_stitch(c)
    assert got['labels'].dtype == np.uint8 and got['tie_risk'].dtype == np.int32 and got['probs'].dtype == np.float32
    assert np.array_equal(got['probs'], probs), c['name']    # (float32 values in float64 compare exactly)
    assert np.array_equal(got['labels'], labels), c['name']
    assert np.array_equal(got['tie_risk'], ties), c['name']
    if c['ties'] is not None:                                # the count each image was built to have
        assert got['tie_risk'].tolist() == c['ties'] and len(set(c['ties'])) == c['n_img'], c['name']
    return got


@pytest.mark.parametrize('name', cases.STITCH_NAMES)
def test_stitch_restatement_equals_the_oracle(name):
    c = cases.make_stitch(name)
    assert c['probs'].shape == (c['n_img'] * cases.n_patches(c['H'], c['W']), 256, 256, int(name[-1])) and np.abs(c['probs'][..., :4]).max() <= 1.0
    got = _check_stitch_against_the_oracle(c)
    if 'rows' in c:                                          # the rows are read back where they were put
        assert np.array_equal(got['probs'][0][c['at']], c['rows'])
        g = np.load(os.path.join(cases.GOLDEN, 'quant_argmax.npz'), allow_pickle=False)
        assert np.array_equal(got['labels'][0][c['at']][-len(g['label']):], g['label'])


def test_stitch_restatement_equals_the_oracle_on_the_batch_over_the_cap():
    c = cases.big_stitch_case()
    assert c['probs'].nbytes == 256 << 20 and c['n_img'] * c['H'] * c['W'] > 16384 * 256 and (c['H'] * c['W']) % 256
    got = _check_stitch_against_the_oracle(c)
    px = c['H'] * c['W']
    model = ref.launch_model(got['ties'], c['n_img'], px)
    print('\n%s: %d additions inside the loop and %d at the end of a mixed workgroup carry a count' % (c['name'], model['loop_flushes'], model['mixed_ends']))
    assert model['loop_flushes'] >= 5 and model['mixed_ends'] >= 64 and np.array_equal(model['tie_risk'], got['tie_risk'])
    first = got['ties'][0].reshape(-1)                       # image 0: workgroups 0 .. 127, then the two parts of workgroup 128
    assert [int(first[lo:hi].sum()) >= n for lo, hi, n in cases.BIG_ZONES] == [True] * 3
    for slip in ('thread0', 'dropped'):                      # and a slip on either path changes a count
        assert not np.array_equal(ref.launch_model(got['ties'], c['n_img'], px, slip)['tie_risk'], got['tie_risk'])


def test_the_launch_paths_the_cases_are_named_for_carry_a_count():
    """The mixed workgroup end (a thread whose image is not that of its workgroup's thread 0 adds its own count) needs near-ties within
    256 pixels of an image boundary, on the far side of it; the flush inside the loop needs them in pixels whose thread walks on into
    another image.  ``launch_model`` counts both for every case."""
    seen = {}
    for name in cases.STITCH_NAMES:
        c = cases.make_stitch(name)
        got = ref.stitch(c['probs'], c['n_img'], c['H'], c['W'])
        m = ref.launch_model(got['ties'], c['n_img'], c['H'] * c['W'])
        assert np.array_equal(m['tie_risk'], got['tie_risk']), name
        seen[name] = (m['loop_flushes'], m['mixed_ends'])
    print('\n%-28s | in the loop | mixed end' % 'case')
    for name, (a, b) in seen.items():
        print('%-28s | %11d | %9d' % (name, a, b))
    for name in ('stitch_257x257_n3_cs4', 'stitch_257x257_n3_cs8', 'stitch_300x462_n3_cs4', 'stitch_300x300_n2_cs4', 'stitch_463x300_n2_cs4'):
        assert seen[name][0] == 0 and seen[name][1] >= 2, name        # (a): workgroups across image boundaries, under the cap
    assert seen['stitch_256x256_n65_cs4'][0] >= 10 and seen['stitch_256x256_n129_cs4'][0] >= 1000         # (b): 2 and 3 images per thread
    assert seen['stitch_256x256_n65_cs4'][1] == seen['stitch_256x256_n129_cs4'][1] == 0                   # ... in aligned workgroups


def test_stitch_cases_cover_what_they_name():
    sizes = {(H, W) for H, W, _ in cases.STITCH_SIZES}
    assert sizes == {(256, 256), (257, 257), (300, 300), (300, 462), (305, 306), (462, 256), (463, 300)}
    assert ref.window_starts(256) == [0] and ref.window_starts(257) == [0, 1] and ref.window_starts(462) == [0, 206]
    assert ref.window_starts(305) == [0, 49] and ref.window_starts(306) == [0, 50] and ref.window_starts(463) == [0, 206, 207]
    never = lambda H, W: int((ref.stitch_map(H, W) < 0).sum())
    assert never(300, 300) == 25 * 44 and never(300, 462) == 0 and never(256, 256) == 25 * 25 * 2 and never(257, 257) == 25      # :242
    for H, W, n in cases.STITCH_BATCHES:                     # threads visit 2 and 3 images; no workgroup holds two images
        assert (H * W) % 256 == 0 and -(-n * H * W // (16384 * 256)) == {65: 2, 129: 3}[n]
    names = [n for n, _ in cases.pixel_rows()]
    assert names[:3] == ['q_and_q_minus_1', 'q_and_q', 'q_and_q_minus_2'] and all(len(r) == 5 * 24 for _, r in cases.pixel_rows()[:3])
    assert {'stitch_257x257_n3_cs8', 'pixel_rows_cs8'} <= set(cases.STITCH_NAMES)
    wide = cases.make_stitch('pixel_rows_cs8')['probs']
    assert wide.shape[-1] == 8 and (wide[..., 4:] == cases.UNUSED).all() and cases.UNUSED > 1


@pytest.mark.parametrize('k', range(len(PRE_CASES)), ids=PRE_NAMES)
def test_preprocess_restatement_equals_the_oracle(k):
    for img in PRE_CASES[k]['imgs']:
        got = ref.preprocess(img)
        plain = img[..., 0] if img.shape[-1] == 1 else img
        assert np.array_equal(got['gray'], o_pre.meta_preprocess(plain))
        g8 = ref.pick_channel(o_pre.u16_to_u8(plain))
        assert np.array_equal(ref.u16_to_u8(plain), o_pre.u16_to_u8(plain))
        assert got['threshold'] == o_pre.otsu_threshold_u8(g8) and np.array_equal(got['hist'], np.bincount(g8.ravel(), minlength=256))
        assert got['inverted'] == int(np.count_nonzero(g8 > got['threshold']) > g8.size * 0.5)


def test_preprocess_cases_cover_what_they_name():
    by = {c['name']: c['imgs'] for c in PRE_CASES}
    assert {c['imgs'].shape[1:3] for c in PRE_CASES} >= set(cases.PRE_EXTENTS)
    assert {(c['imgs'].shape[3], c['imgs'].dtype.name) for c in PRE_CASES} >= {(C, t) for C in (1, 3, 4) for t in ('uint8', 'uint16')}
    assert np.array_equal(np.sort(by['every_u16_value_c1'].ravel()), np.arange(65536))
    assert np.array_equal(by['every_u16_value_c3'][..., 2], by['every_u16_value_c1'][..., 0])
    for H, W in ((16, 16), (17, 15), (256, 256)):
        px = H * W
        for label, upper, inv in (('half', px // 2, 0), ('half_plus_1', px // 2 + 1, 1), ('half_rounded_up', (px + 1) // 2, px % 2)):
            st = ref.preprocess(by['two_valued_%dx%d_%s' % (H, W, label)][0])
            assert int(st['hist'][200]) == upper and int(st['hist'][40]) == px - upper and 40 <= st['threshold'] < 200 and st['inverted'] == inv
    for n in (1, 64, 65, 129):
        flags = [ref.preprocess(im)['inverted'] for im in by['alternating_batch_of_%d' % n]]
        assert flags == [k % 2 for k in range(n)]
    for value in (0, 1, 255):
        assert ref.preprocess(by['constant_%d' % value][0])['threshold'] == 0
        assert ref.preprocess(by['constant_%d' % value][0])['inverted'] == int(value > 0)


# ---- the histograms ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hists():
    names, hs, px = cases.otsu_histograms()
    plain = [ref.otsu_decide(h, int(p)) for h, p in zip(hs, px)]
    fused = [ref.otsu_decide(h, int(p), ref.otsu_fused) for h, p in zip(hs, px)]
    return names, hs, px, plain, fused


def test_histogram_restatement_equals_the_oracle(hists):
    names, hs, px, plain, _ = hists
    assert len(names) == len(set(names)) and (hs.sum(axis=1) == px).all() and px.max() == cases.INT32_MAX and px.min() == 1
    seen = 0
    for name, h, p, (t, inv) in zip(names, hs, px, plain):
        if p > 2 * 10 ** 7:                                  # (the oracle takes an image: the largest counts have none)
            continue
        img = np.repeat(np.arange(256, dtype=np.uint8), h)[None]
        assert t == o_pre.otsu_threshold_u8(img), name
        assert inv == int(np.count_nonzero(img > t) > img.size * 0.5), name
        seen += 1
    assert seen >= len(names) - 8
    eps = ref.FLT_EPSILON                                    # one pixel against 2^23 - 1 has the weight FLT_EPSILON itself: kept
    assert 1e-6 > eps == 2.0 ** -23 > 1 / (2 ** 23 + 1) > 1 / (10 ** 7 + 1) and eps == float(np.finfo(np.float32).eps)
    by = dict(zip(names, plain))
    assert [by['one_pixel_below_' + k][0] for k in ('1e6', '2p23_minus_1', '2p23', '1e7', '1e8', 'int32_max_minus_1')] == [3, 3, 0, 0, 0, 0]
    assert [by['one_pixel_above_' + k][0] for k in ('1e6', '2p23_minus_1', '2p23', '1e7', '1e8', 'int32_max_minus_1')] == [3, 3, 0, 0, 0, 0]
    assert by['single_bin_0'] == (0, 0) and by['single_bin_255'] == (0, 1)


def test_condition_fused_otsu_decides_otherwise_on_100_histograms_or_more(hists):
    names, _, _, plain, fused = hists
    thr = [n for n, a, b in zip(names, plain, fused) if a[0] != b[0]]
    flag = [n for n, a, b in zip(names, plain, fused) if a[1] != b[1]]
    families = sorted({n.rsplit('_', 1)[0] for n in flag})
    print('\n%d histograms (seed %d): fused and plain Otsu disagree on the threshold of %d and on the inversion flag of %d (%s)'
          % (len(names), cases.HIST_SEED, len(thr), len(flag), ', '.join('%s: %d' % (f, sum(n.startswith(f) for n in flag)) for f in families)))
    assert len(flag) >= 100


# ---- the mutants ------------------------------------------------------------------------------------------------------------------
def _pre_differs(**kw):
    """The preprocess cases on which a mutant of ``ref.preprocess`` changes a stage product."""
    out = []
    for c in PRE_CASES:
        for img in c['imgs']:
            a, b = ref.preprocess(img), ref.preprocess(img, **kw)
            if any(not np.array_equal(a[key], b[key]) for key in ref.PRE_ORDER):
                out.append(c['name'])
                break
    return out


def _stitch_differs(names, **kw):
    out = []
    for name in names:
        c = cases.make_stitch(name)
        a, b = ref.stitch(c['probs'], c['n_img'], c['H'], c['W']), ref.stitch(c['probs'], c['n_img'], c['H'], c['W'], **kw)
        if any(not np.array_equal(a[key], b[key]) for key in ref.STITCH_ORDER):
            out.append(name)
    return out


def test_every_mutant_is_caught_by_a_named_case(hists):
    names, _, _, plain, fused = hists
    small = cases.SMALL_STITCH_NAMES
    rows = [
        ('otsu_fused: the two products contracted', [n for n, a, b in zip(names, plain, fused) if a != b]),
        ('>= for > in the white decision', _pre_differs(or_equal=True)),
        ('channel 0 for channel 2', _pre_differs(channel=0)),
        ('truncation in u16 -> u8', _pre_differs(truncate=True)),
        ('the tie test < 1 for <= 1', _stitch_differs(small, gap=0)),
        ('the last maximum for the first', _stitch_differs(small, last=True)),
        ('counters summed modulo 64 images', _stitch_differs(small + ['stitch_256x256_n65_cs4'], count_modulo=64)),
        ("a mixed workgroup's other image counted for thread 0's", _stitch_differs(small, end_of_other_image='thread0')),
        ("a mixed workgroup's other image not counted", _stitch_differs(small, end_of_other_image='dropped')),
    ]
    print('\n%-55s | cases that catch it' % 'mutant')
    for name, caught in rows:
        print('%-55s | %d: %s%s' % (name, len(caught), ', '.join(caught[:4]), ', ...' if len(caught) > 4 else ''))
        assert caught, 'no case shows: ' + name
    by = dict(rows)
    assert any(n.startswith('two_valued_') and n.endswith('_half') for n in by['>= for > in the white decision'])
    assert by['counters summed modulo 64 images'] == ['stitch_256x256_n65_cs4']      # (64 images or fewer fold onto themselves)
    for key in ("a mixed workgroup's other image counted for thread 0's", "a mixed workgroup's other image not counted"):
        assert {'stitch_257x257_n3_cs4', 'stitch_300x462_n3_cs4', 'stitch_257x257_n3_cs8'} <= set(by[key])
    assert {'pixel_rows_cs4', 'pixel_rows_cs8'} <= set(by['the tie test < 1 for <= 1']) & set(by['the last maximum for the first'])


def test_round_half_up_in_u16_to_u8_is_no_mutant_at_all():
    """Round-half-up for cvRound's half-to-even changes NO uint16 value, so no case can catch it, and the device is free to round
    either way: the float32 product v * float32(255 / 65535) of every one of the 65536 values lies 0.0019 or more from a half
    (v / 257 comes no closer than 0.5 / 257 to one, and the two float32 roundings move it by 2e-5 at the most).  Shown over the whole
    domain, which 'every_u16_value' runs on the device; the mutant table holds truncation in its place."""
    v = np.arange(65536, dtype=np.uint16)
    f = (v.astype(np.float32) * np.float32(255.0 / 65535.0)).astype(np.float64)
    gap = float(np.abs(f - np.floor(f) - 0.5).min())
    print('\nround-half-up against half-to-even in u16 -> u8: 0 of 65536 values differ; the closest product to a half is %.6f away' % gap)
    assert gap > 0.0019 and np.array_equal(ref.u16_to_u8(v, half_up=True), ref.u16_to_u8(v)) and f.max() == 255.0
    assert int((ref.u16_to_u8(v, truncate=True) != ref.u16_to_u8(v)).sum()) == 32640
