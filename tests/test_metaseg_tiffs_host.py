"""The ``tiff_read_on_device`` key of ``make metaseg`` without a GPU: the configuration errors, the four entry points of the C ABI in
the header and in the built library, and - on an injected handle that decodes with the host reader - which batches the driver
sends to ``meta_segment_tiffs`` and which stay with ``meta_segment``."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_decode_cases as tc                                          # noqa: E402
from test_host_multirank import StubHandle, StubModel, make_inputs     # noqa: E402
from ecseg_amd import image_io, metaseg      # noqa: E402
from ecseg_amd._lib import EXPORTS, load_library      # noqa: E402
from ecseg_amd.utils import get_imgs         # noqa: E402
from oracle import postproc                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ecseg_meta_segment_tiffs', 'ecseg_meta_segment_tiffs_files', 'ecseg_prefetch_tiffs', 'ecseg_get_read_timings')
H, W = 96, 128


def test_the_key_must_be_a_boolean_and_needs_a_handle_with_the_call(tmp_path, monkeypatch, capsys):
    inp = tmp_path / 'images'
    make_inputs(str(inp), 1)
    monkeypatch.chdir(tmp_path)
    for value in ('yes', 1, 'true', [True]):
        yaml.safe_dump({'metaseg': {'inpath': str(inp), 'tiff_read_on_device': value}}, open(tmp_path / 'config.yaml', 'w'))
        with pytest.raises(SystemExit) as e:
            metaseg.main([])
        assert e.value.code == 2 and 'tiff_read_on_device must be true or false' in capsys.readouterr().out
    with pytest.raises(ValueError, match='tiff_read_on_device'):
        metaseg.run(str(inp), StubModel(), get_imgs(str(inp)), 0, 1, batch_images=2, io_threads=2, log=lambda *a: None, tiff_read_on_device=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    text = open(os.path.join(ROOT, 'config.yaml')).read()
    assert 'tiff_read_on_device' not in cfg['metaseg'] and '# tiff_read_on_device' in text[text.index('\nmetaseg:'):text.index('\nfish_distance_calculation:')]


def test_the_four_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    lib = load_library()
    for name in NEW:
        assert 'int %s(' % name in header, name
        assert name in EXPORTS and getattr(lib, name) is not None, name
    assert 'int ecseg_get_file_timings(ecseg_ctx* h, float* ms_out /* [2] */);' in header     # (old callers pass two floats)


class TiffsHandle(StubHandle):
    """A handle with the device call of ``tiff_read_on_device``: the files are decoded by the host reader, the rest is the stub's."""

    def __init__(self, tmp, **kw):
        super().__init__(**kw)
        self.tmp, self.tiffs, self.plain, self.named = str(tmp), [], [], []

    def _labels(self, imgs):
        gray, _ = self.preprocess(imgs)
        post = (gray >> 6).astype(np.uint8)
        return gray, post, np.array([postproc.count_cc(p == 3)[0] for p in post], np.int32), np.zeros(len(gray), np.int32)

    def meta_segment(self, imgs, gray_out=None, post_out=None):
        self.plain.append(len(imgs))
        return self._labels(imgs)

    def meta_segment_tiffs(self, datas, shape, gray_out=None, post_out=None):
        imgs = []
        for d in datas:
            p = os.path.join(self.tmp, 'one.tif')
            open(p, 'wb').write(bytes(d))
            imgs.append(image_io._native_tiff(p))
        assert all(im.shape[:2] == tuple(shape[:2]) for im in imgs)
        self.tiffs.append(len(datas))
        return self._labels(np.stack(imgs)) + ([0] * len(datas),)

    def prefetch_tiffs(self, datas, shape=None):
        self.named.append(None if datas is None else len(datas))

    def read_timings(self):
        return {'decode': 0.0}


def _lzw_file(img, rps=1):
    rows = img.reshape(img.shape[0], -1)
    strips = [tc.pack(tc.lzw_codes(rows[r:r + rps].tobytes())) for r in range(0, len(rows), rps)]
    return tc.tiff_file(strips, img.shape[0], img.shape[1], rps, spp=1 if img.ndim == 2 else img.shape[2])


def _folder(folder):
    """12 + 3 LZW files at one row per strip (96 strips each: a batch of 12 passes the rule's 1040 strips, the 3 behind it do not), a
    Deflate file and a .npy image, all 96 x 128 RGB"""
    from PIL import Image
    os.makedirs(folder)
    rng = np.random.default_rng(5)
    for name in ['a%02d.tif' % i for i in range(12)] + ['b0.tif', 'b1.tif', 'b2.tif', 'c0.tif', 'd0.npy']:
        img = np.zeros((H, W, 3), np.uint8)
        img[..., 2] = rng.integers(0, 64, (H, W))
        y, x = rng.integers(4, H - 8), rng.integers(4, W - 8)
        img[y:y + 3, x:x + 4, 2] = 250
        p = os.path.join(folder, name)
        if name.endswith('.npy'):
            np.save(p, img)
        elif name[0] == 'c':
            Image.fromarray(img).save(p, compression='tiff_adobe_deflate')
        else:
            open(p, 'wb').write(_lzw_file(img))
    for sub in ('dapi', 'labels'):
        os.makedirs(os.path.join(folder, sub))


def _tree(folder):
    return {os.path.join(sub, n): open(os.path.join(folder, sub, n), 'rb').read() for sub in ('dapi', 'labels')
            for n in sorted(os.listdir(os.path.join(folder, sub)))}


def test_the_grouping_sends_accepted_sets_of_lzw_files_to_the_device_and_the_rest_to_the_host(tmp_path):
    off, on = str(tmp_path / 'off'), str(tmp_path / 'on')
    _folder(off)
    _folder(on)
    quiet = lambda *a: None
    base = StubModel()
    base.handle = TiffsHandle(tmp_path)
    rec_off = metaseg.run(off, base, get_imgs(off), 0, 1, batch_images=12, io_threads=2, log=quiet)
    assert base.handle.tiffs == [] and sum(base.handle.plain) == 17
    model, stats = StubModel(), {}
    model.handle = TiffsHandle(tmp_path)
    rec_on = metaseg.run(on, model, get_imgs(on), 0, 1, batch_images=12, io_threads=2, log=quiet, stats=stats, tiff_read_on_device=True)
    assert np.array_equal(rec_off, rec_on) and (rec_on[:, 1] == 0).all()
    # the twelve files that pass the rule together went as files; the refused set of three as images, and so the Deflate file and the
    # .npy, which share a batch (one shape, one route)
    assert model.handle.tiffs == [12] and sorted(model.handle.plain) == [2, 3]
    assert stats['tiff_device_images'] == 12
    assert _tree(off) == _tree(on) and len(_tree(on)) == 17 * 3
    # with emit_probs the key is without effect (its device call takes decoded images): nothing reaches meta_segment_tiffs
    again = StubModel()
    again.handle = TiffsHandle(tmp_path)
    again.segment_ex = lambda gray, want_probs=False: again.segment(gray) + (np.zeros(len(gray), np.int32), np.zeros(gray.shape + (4,), np.float32))
    metaseg.run(on, again, get_imgs(on)[:12], 0, 1, batch_images=12, io_threads=2, log=quiet, emit_probs=True, tiff_read_on_device=True)
    assert again.handle.tiffs == []


def test_a_file_the_device_refuses_goes_to_the_host_reader_alone(tmp_path):
    folder = str(tmp_path / 'x')
    _folder(folder)
    paths = get_imgs(folder)[:12]

    class Refusing(TiffsHandle):
        def meta_segment_tiffs(self, datas, shape, gray_out=None, post_out=None):
            gray, post, nec, tie, st = super().meta_segment_tiffs(datas, shape)
            st[3], st[7] = -5, -1                                        # (ECSEG_E_UNSUPPORTED after all; a stream the device finds corrupt)
            gray[3] = gray[7] = 0
            nec[3] = nec[7] = -1
            return gray, post, nec, tie, st
    want = StubModel()
    want.handle = TiffsHandle(tmp_path)
    rec_want = metaseg.run(folder, want, paths, 0, 1, batch_images=12, io_threads=2, log=lambda *a: None)
    tree = _tree(folder)
    model, stats = StubModel(), {}
    model.handle = Refusing(tmp_path)
    rec = metaseg.run(folder, model, paths, 0, 1, batch_images=12, io_threads=2, log=lambda *a: None, stats=stats, tiff_read_on_device=True)
    assert np.array_equal(rec, rec_want) and _tree(folder) == tree       # (the host reads both files: the records and the outputs are whole)
    assert model.handle.tiffs == [12] and model.handle.plain == [1, 1] and stats['tiff_device_images'] == 10
