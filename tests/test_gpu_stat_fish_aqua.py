"""ecseg_fish_render (csrc/fishspot_kernels.hip) and the third FISH probe of ``make stat_fish`` on the device.  The three colour
rasters are compared byte for byte with the restatement tests/aqua_ref.py, which evaluates the reference's own expression (its
uint8 wrap included), never with the product's numpy path - except where the point is that the two paths write the same files."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aqua_ref                              # noqa: E402
import test_stat_fish_aqua as cpu            # noqa: E402
from ecseg_amd import csvio                  # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

pytestmark = pytest.mark.gpu
ORDERS = {3: ((0, 1, 2), (2, 1, 0)), 4: ((0, 1, 2, 3), (2, 1, 0, 3), (3, 0, 2, 1))}


def _check(gpu, I, channels, thr, bnd):
    """``I``: the image as the reference indexes it, BGR(A); the device gets it with reference channel k in channel channels[k]."""
    img = np.empty_like(I)
    img[..., list(channels)] = I
    got = gpu.fish_render(img, channels, thr, bnd)
    want = aqua_ref.files(I, thr, bnd)
    for g, w, what in zip(got, want, ('original', 'with_segmentation', 'lsq')):
        assert g.dtype == np.uint8 and g.shape == w.shape
        assert g.tobytes() == w.tobytes(), '%s differs in %d byte(s), channels %s' % (what, int((g != w).sum()), channels)


def _masks(rng, H, W, n_probe, boundaries):
    thr = (rng.random((H, W, n_probe)) < 0.4).astype(np.uint8) * np.uint8(255)
    bnd = {'off': np.zeros((H, W), np.uint8), 'on': np.full((H, W), 255, np.uint8),
           'mixed': (rng.random((H, W)) < 0.5).astype(np.uint8) * np.uint8(255)}[boundaries]
    return thr, bnd


@pytest.mark.parametrize('boundaries', ['off', 'on', 'mixed'])
def test_every_colour_and_aqua_value_under_every_coefficient(gpu, boundaries):
    I = aqua_ref.exhaustive_image()
    thr, bnd = _masks(np.random.default_rng(7), 256, 256, 3, boundaries)
    for channels in ORDERS[4]:
        _check(gpu, I, channels, thr, bnd)
    for channels in ORDERS[3]:
        _check(gpu, np.ascontiguousarray(I[..., :3]), channels, np.ascontiguousarray(thr[..., :2]), bnd)


def test_the_sixteen_combinations_of_the_lsq_merge(gpu):
    bnd, thr = aqua_ref.lsq_combinations()
    I = np.random.default_rng(1).integers(0, 256, (4, 4, 4), dtype=np.uint8)
    _check(gpu, I, (0, 1, 2, 3), thr, bnd)
    lsq = gpu.fish_render(I, (0, 1, 2, 3), thr, bnd)[2]
    assert lsq[3, 3].tolist() == [255, 255, 255] and lsq[2, 0].tolist() == [233, 137, 54]      # everything set; the aqua mask alone (RGB)
    # any byte is taken as a mask value: the floor of coeff * mask / 255 (the boundaries stay 0 / 255, as ecseg_fish_spots writes them)
    rng = np.random.default_rng(2)
    _check(gpu, I, (0, 1, 2, 3), rng.integers(0, 256, (4, 4, 3), dtype=np.uint8), bnd)


@pytest.mark.parametrize('C', [3, 4])
@pytest.mark.parametrize('size', [(1, 1), (1, 7), (5, 1), (67, 93)])
def test_extents_that_are_no_multiple_of_a_vector(gpu, size, C):
    H, W = size
    rng = np.random.default_rng(H * 1000 + W + C)
    I = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if C == 4:                                               # the two aqua values at which the wrap shows, and saturated colours under them
        I[..., 3].flat[::3] = cpu.Q_GREEN
        I[..., 3].flat[1::3] = cpu.Q_RED
        I[..., :3].flat[::5] = 255
    for boundaries in ('off', 'on', 'mixed'):
        thr, bnd = _masks(rng, H, W, C - 1, boundaries)
        for channels in ORDERS[C]:
            _check(gpu, I, channels, thr, bnd)


def test_argument_errors_leave_the_handle_usable(gpu):
    from ecseg_amd._lib import EcsegError, _ptr
    rng = np.random.default_rng(4)
    H, W = 6, 9
    out = [np.empty((H, W, 3), np.uint8) for _ in range(3)]
    bnd = np.zeros((H, W), np.uint8)
    small = np.zeros(64, np.uint8)

    def call(C, channels, n_probe, h=H, w=W):
        img = np.zeros((H, W, max(C, 1)), np.uint8)
        thr = np.zeros((H, W, max(n_probe, 1)), np.uint8)
        ch = np.array(channels, np.int32)
        return gpu.lib.ecseg_fish_render(gpu.h, _ptr(img), h, w, C, _ptr(ch), _ptr(thr), n_probe, _ptr(bnd), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]))

    for args, text in (((2, (0, 1), 1), '3 or 4 channels'), ((5, (0, 1, 2, 3, 4), 4), '3 or 4 channels'),
                       ((3, (0, 1, 2), 3), 'n_probe'), ((4, (0, 1, 2, 3), 2), 'n_probe'), ((4, (0, 1, 2, 3), 4), 'n_probe'),
                       ((3, (0, 1, 3), 2), 'channel index'), ((3, (-1, 1, 2), 2), 'channel index'), ((4, (0, 1, 2, 4), 3), 'channel index')):
        assert call(*args) == -1, args
        assert text in gpu.lib.ecseg_last_error(gpu.h).decode(), args
        I = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        _check(gpu, I, (0, 1, 2, 3), *_masks(rng, H, W, 3, 'mixed'))
    # H * W = 2^31: refused before anything is read
    ch = np.array([0, 1, 2], np.int32)
    assert gpu.lib.ecseg_fish_render(gpu.h, _ptr(small), 65536, 32768, 3, _ptr(ch), _ptr(small), 2, _ptr(small), _ptr(small), _ptr(small), _ptr(small)) == -1
    assert 'too large' in gpu.lib.ecseg_last_error(gpu.h).decode()
    with pytest.raises(EcsegError) as e:
        gpu.fish_render(np.zeros((H, W, 4), np.uint8), (0, 1, 2, 3), np.zeros((H, W, 2), np.uint8), bnd)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        gpu.fish_render(np.zeros((H, W, 4), np.uint8), (0, 1, 2), np.zeros((H, W, 3), np.uint8), bnd)
    _check(gpu, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (2, 1, 0), *_masks(rng, H, W, 2, 'mixed'))
    assert 0 < gpu.timings()['count'] < 1000


@pytest.mark.parametrize('seed', [403, 405])
def test_three_probes_through_process_image(gpu, tmp_path, seed):
    img, mask = cpu.four_channel_scene(seed, (120, 140))
    from ecseg_amd import image_io
    np.save(tmp_path / 's.npy', img)
    image_io.write_tiff_gray8(str(tmp_path / 's_mask.tif'), mask)
    params = dict(sf.DEFAULT_PARAMS, color_sensitivity=[70, 70, 70])
    stats = {}
    rows, scale = sf.process_image(str(tmp_path / 's.npy'), str(tmp_path / 's_mask.tif'), str(tmp_path / 'out'), params, 1, gpu, stats=stats)
    want_rows, lab, want_files, rec = cpu.expected('s', img, mask)
    assert stats['probes'] == 3 and scale == 1 and rows == want_rows and rec[:, 15].sum() > 10
    for got, want in zip(cpu.read_outputs(tmp_path / 'out', 's'), want_files):
        assert np.array_equal(got, want)
    assert np.array_equal(np.load(tmp_path / 'out' / 's' / 's__segmentation_min_cut.npy'), lab)


def test_main_on_a_four_channel_folder_equals_the_oracle_run(gpu, tmp_path, monkeypatch):
    inp, scenes = cpu.make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=cpu.OracleHandle())
    want = cpu.folder_bytes(inp / 'annotated')
    sf.main([], handle=gpu)
    got = cpu.folder_bytes(inp / 'annotated')
    assert sorted(got) == sorted(want) and len(want) == 3 * 5 + 2
    for name in want:
        assert got[name] == want[name], name
    rows = sum((cpu.expected(name, *scenes[name])[0] for name in cpu.ORDER), [])
    assert got['stat_fish_lsq.csv'].decode() == csvio.csv_text(cpu.COLUMNS_3, rows)


def test_a_three_channel_folder_is_byte_identical_to_the_numpy_path(gpu, tmp_path, monkeypatch):
    """Routing every image through fish_render changes nothing: the same handle without the method takes the numpy path."""
    class WithoutRender:
        def __getattr__(self, name):
            if name == 'fish_render':
                raise AttributeError(name)
            return getattr(gpu, name)

    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'), ('two', 'tif')), size=(67, 93), color_sensitivity=(70, 70))
    monkeypatch.chdir(tmp_path)
    assert not hasattr(WithoutRender(), 'fish_render') and hasattr(gpu, 'fish_render')
    sf.main([], handle=WithoutRender())
    want = cpu.folder_bytes(inp / 'annotated')
    sf.main([], handle=gpu)
    got = cpu.folder_bytes(inp / 'annotated')
    assert sorted(got) == sorted(want) and len(want) == 2 * 5 + 2
    for name in want:
        assert got[name] == want[name], name
    assert any('_lsq_n15_std3.00_s7_g70.0_r70.0.tif' in name for name in want)
