"""The host label-PNG coder after its split (csrc/png_label_code.h holds the code build that deflate_labels and the device coder's
driver share): every file of tests/png_label_cases.py has the bytes the coder wrote before the split, inflates to the palette rows,
and has the size the counts alone give.  And the ``files_on_device`` key of ``make metaseg`` on injected handles."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_cases as pc                 # noqa: E402
from ecseg_amd import image_io, metaseg      # noqa: E402
from ecseg_amd._lib import load_library      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FILES = {}


def host_file(case, tmp_path_factory):
    if case.name not in _FILES:
        path = str(tmp_path_factory.mktemp('png') / 'l.png')
        image_io.write_label_png(path, case.labels)
        _FILES[case.name] = open(path, 'rb').read()
    return _FILES[case.name]


def chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body)
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def test_the_case_list_covers_what_it_names():
    shapes = {c.labels.shape for c in pc.CASES}
    assert {(H, W) for H in pc.HEIGHTS for W in pc.WIDTHS} <= shapes and (520, 696) in shapes and (300, 270) in shapes
    assert any(c.labels.shape[1] == 1 and len(np.unique(c.labels)) == 1 for c in pc.CASES)          # no match at all
    assert any(c.labels.max() > 3 for c in pc.CASES)
    assert len(pc.CASES) == len({c.name for c in pc.CASES})
    assert len({im.tobytes() for im in pc.batch(5)}) == 5


def test_the_split_of_the_host_coder_changed_no_byte(tmp_path_factory):
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'png_labels_sha256.json')))
    assert sorted(want) == sorted(c.name for c in pc.CASES)
    for c in pc.CASES:
        assert hashlib.sha256(host_file(c, tmp_path_factory)).hexdigest() == want[c.name], c.name


def test_every_file_inflates_to_the_palette_rows(tmp_path_factory):
    for c in pc.CASES:
        H, W = c.labels.shape
        ch = chunks(host_file(c, tmp_path_factory))
        assert [t for t, _ in ch] == [b'IHDR', b'IDAT', b'IEND'], c.name
        assert ch[0][1] == struct.pack('>IIBBBBB', W, H, 8, 6, 0, 0, 0), c.name
        assert ch[1][1][:2] == b'\x78\x01' and zlib.decompress(ch[1][1]) == pc.expected_rows(c.labels), c.name


def test_the_size_from_the_counts_is_the_size_of_the_stream(tmp_path_factory):
    lib = load_library()
    for c in pc.CASES:
        H, W = c.labels.shape
        lab = np.ascontiguousarray(c.labels)
        formula, written = C.c_longlong(), C.c_longlong()
        assert lib.ecseg_png_labels_stream_size(lab.ctypes.data_as(C.c_void_p), H, W, C.byref(formula), C.byref(written)) == 0
        idat = chunks(host_file(c, tmp_path_factory))[1][1]
        assert formula.value == written.value == len(idat), c.name
    assert lib.ecseg_png_labels_stream_size(None, 4, 4, C.byref(formula), C.byref(written)) == -1


# ---- the files_on_device key of `make metaseg` on injected handles ----------------------------------------------------------------
from test_host_multirank import StubHandle, StubModel, make_inputs     # noqa: E402
from ecseg_amd.utils import get_imgs         # noqa: E402
from oracle import postproc                  # noqa: E402


class FilesHandle(StubHandle):
    """A handle with the device call of ``files_on_device``: marked bytes stand for the files it produces, None for those it does
    not (``drop``: per kind the numbers, in call order, of the images without a file)."""

    def __init__(self, drop=None, **kw):
        super().__init__(**kw)
        self.drop = drop or {'dapi': (), 'png': ()}
        self.seen = 0
        self.capacities = []

    def meta_segment_files(self, imgs, gray_out=None, post_out=None, dapi_capacity=None, png_capacity=None, file_bufs=None):
        gray, _ = self.preprocess(imgs)
        post = (gray >> 6).astype(np.uint8)
        nec = np.array([postproc.count_cc(p == 3)[0] for p in post], np.int32)
        self.capacities.append((imgs.shape[1:3], dapi_capacity, png_capacity))
        files = {}
        for kind in ('dapi', 'png'):
            files[kind] = [None if self.seen + j in self.drop[kind] else ('device %s %d' % (kind, self.seen + j)).encode() for j in range(len(imgs))]
        self.seen += len(imgs)
        return gray, post, nec, np.zeros(len(imgs), np.int32), files['dapi'], files['png']


def _tree(folder):
    out = {}
    for sub in ('dapi', 'labels'):
        for name in sorted(os.listdir(os.path.join(folder, sub))):
            out[sub + '/' + name] = open(os.path.join(folder, sub, name), 'rb').read()
    return out


def test_a_file_the_device_did_not_produce_is_written_by_the_host_writer(tmp_path):
    off, on = str(tmp_path / 'off'), str(tmp_path / 'on')
    make_inputs(off, 5)
    make_inputs(on, 5)
    quiet = lambda *a: None
    rec_off = metaseg.run(off, StubModel(), get_imgs(off), 0, 1, batch_images=2, io_threads=2, log=quiet)
    model = StubModel()
    model.handle = FilesHandle(drop={'dapi': (1,), 'png': (2, 4)})
    rec_on = metaseg.run(on, model, get_imgs(on), 0, 1, batch_images=2, io_threads=2, log=quiet, files_on_device=True)
    assert np.array_equal(rec_off, rec_on)
    assert model.handle.capacities == [((96, 128), 96 * 128 + 65536, 96 * 128 // 2 + 65536)] * 3
    want, got = _tree(off), _tree(on)
    assert sorted(want) == sorted(got) and len(want) == 5 * 3
    for i in range(5):
        dapi, png, npy = 'dapi/img%02d.tif' % i, 'labels/img%02d.png' % i, 'labels/img%02d.npy' % i
        assert got[dapi] == (want[dapi] if i == 1 else b'device dapi %d' % i)
        assert got[png] == (want[png] if i in (2, 4) else b'device png %d' % i)
        assert got[npy] == want[npy]
    assert not [n for sub in ('dapi', 'labels') for n in os.listdir(os.path.join(on, sub)) if '.tmp' in n]


def test_emit_probs_and_a_dapi_name_that_is_no_tiff_keep_the_host_writers(tmp_path):
    folder = tmp_path / 'x'
    for sub in ('dapi', 'labels'):
        os.makedirs(folder / sub)
    gray = np.arange(96 * 128, dtype=np.uint8).reshape(96, 128)
    post = gray >> 6
    metaseg._write_outputs(str(folder / 'a.png'), gray, post, lambda *a: None, None, (b'never written', b'device png'))
    from PIL import Image
    assert np.array_equal(np.array(Image.open(str(folder / 'dapi' / 'a.png'))), ~gray)       # (save_img's file, not the device's bytes)
    assert open(folder / 'labels' / 'a.png', 'rb').read() == b'device png'
    metaseg._write_outputs(str(folder / 'b.tif'), gray, post, lambda *a: None, None, None)
    metaseg._write_outputs(str(folder / 'c.tif'), gray, post, lambda *a: None, None, (None, None))
    for sub, name in (('dapi', '%s.tif'), ('labels', '%s.png'), ('labels', '%s.npy')):
        assert open(folder / sub / (name % 'b'), 'rb').read() == open(folder / sub / (name % 'c'), 'rb').read()


def test_files_on_device_must_be_a_boolean_and_needs_a_handle_with_the_call(tmp_path, monkeypatch, capsys):
    inp = tmp_path / 'images'
    make_inputs(str(inp), 1)
    monkeypatch.chdir(tmp_path)
    for value in ('yes', 1, 'true', [True]):
        yaml.safe_dump({'metaseg': {'inpath': str(inp), 'files_on_device': value}}, open(tmp_path / 'config.yaml', 'w'))
        with pytest.raises(SystemExit) as e:
            metaseg.main([])
        assert e.value.code == 2 and 'files_on_device must be true or false' in capsys.readouterr().out
    with pytest.raises(ValueError, match='files_on_device'):
        metaseg.run(str(inp), StubModel(), get_imgs(str(inp)), 0, 1, batch_images=2, io_threads=2, log=lambda *a: None, files_on_device=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    assert 'files_on_device' not in cfg['metaseg'] and '# files_on_device' in open(os.path.join(ROOT, 'config.yaml')).read()
