"""The batched device TIFF reader without a GPU: the new symbols, the layout function against a restatement, the routing rule for a
set of files, ``image_io.imread_many`` on injected handles, the ``tiff_read_batch`` key of ``make stat_fish``, and the layout and
the batched strip walk of tiffb_unstrip_kernel compiled for the host under ASan + UBSan (tools/asan/tiff_decode_batch_fuzz.cpp)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_decode_cases as dc               # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_documents_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert ('int ecseg_tiff_decode_batch(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges /* [n][2] offset, n_bytes */,\n'
            '                            int n_files, void* dst, long long dst_bytes, const int64_t* dst_offsets /* [n] */,\n'
            '                            int32_t* shapes /* [n][4] H, W, spp, bits */, int32_t* status /* [n] */);') in hdr
    assert 'long long ecseg_tiff_decode_batch_bytes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds);' in hdr
    assert 'int ecseg_tiff_decode_batch_routes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds);' in hdr
    assert 'still 5 - additive: ecseg_tiff_decode_batch' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'still 5 - additive: ecseg_tiff_decode and ecseg_tiff_decode_routes' in hdr          # the earlier lines stay
    lib = _lib.load_library()
    for name in ('ecseg_tiff_decode_batch', 'ecseg_tiff_decode_batch_bytes', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_batch_counts'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(_lib.Handle, 'tiff_decode_many') and hasattr(image_io, 'imread_many')
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_read_batch' in text and 'ecseg_tiff_decode_batch' in text, doc
    assert 'asan_tiff_decode_batch:' in open(os.path.join(ROOT, 'Makefile')).read()
    kernels = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_decode_kernels.hip')).read()
    for k in ('tiffb_unstrip_kernel', 'tiffb_unpredict_kernel', 'tiffb_status_kernel'):
        assert k in kernels, k
    assert 'static_assert(sizeof(TdFile) == 80' in open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_decode_batch.h')).read()


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------
def _build_fuzz(tmp, cxx, san):
    exe = str(tmp / ('tiff_decode_batch_fuzz' + ('_san' if san else '')))
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(ROOT, 'ecseg_amd', 'csrc', 'host_codec.cpp'), os.path.join(ROOT, 'tools', 'asan', 'tiff_decode_batch_fuzz.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope='module')
def fuzz_builds(tmp_path_factory):
    """(the program built with the sanitizers, or None where the host compiler cannot link their runtimes; a plain build then)."""
    tmp = tmp_path_factory.mktemp('batch_fuzz')
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp / 'probe')], capture_output=True, timeout=120).returncode != 0:
        return None, _build_fuzz(tmp, cxx, [])
    return _build_fuzz(tmp, cxx, san), None


@pytest.fixture(scope='module')
def fuzz_exe(fuzz_builds):
    if fuzz_builds[0] is None:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    return fuzz_builds[0]


@pytest.fixture(scope='module')
def layout_exe(fuzz_builds):
    """The layout needs no sanitizer: the plain build serves where there is no other."""
    return fuzz_builds[0] or fuzz_builds[1]


def test_the_batched_walk_equals_the_host_decoder_under_the_sanitizers(fuzz_exe):
    """The stand-alone program (its own main, no preloaded runtime): 400 packed batches with corrupt and truncated files."""
    run = subprocess.run([fuzz_exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_decode_batch_fuzz ok' in run.stdout and ' 0 corrupt files' not in run.stdout, run.stdout


# ---- the layout function against a restatement ----------------------------------------------------------------------------------
KEYS = ('src_off', 'n_bytes', 'dst_off', 'n_table', 'H', 'W', 'spp', 'bps', 'rps', 'lzw', 'swap', 'predictor', 'in_batch')


def _f(src_off, n_bytes, dst_off, H, W, spp=1, bps=1, rps=1, n_table=None, lzw=1, swap=0, predictor=0, in_batch=1):
    nstrips = -(-H // rps)
    return dict(src_off=src_off, n_bytes=n_bytes, dst_off=dst_off, n_table=nstrips if n_table is None else n_table, H=H, W=W, spp=spp, bps=bps,
                rps=rps, lzw=lzw, swap=swap, predictor=predictor, in_batch=in_batch)


def _restated(files):
    """What td_batch_layout and tiff_decode_batch_bufs give, from their description alone: the upload is the span of the files that
    take part, the rasters lie as in the destination from an even base, strip tables are offsets then counts, back to back, the
    grids are running sums, and the arena holds six slots on multiples of 256 bytes (a slot of nothing still takes 256)."""
    part = [f for f in files if f['in_batch']]
    raster = lambda f: f['H'] * f['W'] * f['spp'] * f['bps']
    for f in part:
        if f['bps'] == 2 and f['dst_off'] % 2:
            return None
    src_base = min([f['src_off'] for f in part], default=0)
    src_end = max([f['src_off'] + f['n_bytes'] for f in part], default=0)
    dst_base = min([f['dst_off'] for f in part], default=0) // 2 * 2
    dst_end = max([f['dst_off'] + raster(f) for f in part], default=0)
    rows, strips, rowsum, words = [], 0, 0, 0
    u8 = u16 = 0
    for f in files:
        if f['in_batch']:
            rows.append((f['src_off'] - src_base, words, f['dst_off'] - dst_base, strips, rowsum, 1))
            words += 2 * f['n_table']
            strips += -(-f['H'] // f['rps'])
            rowsum += f['H']
            u16 |= f['bps'] == 2 and bool(f['swap'] or f['predictor'])
            u8 |= f['bps'] == 1 and bool(f['predictor'])
        else:
            rows.append((0, words, 0, strips, rowsum, 0))
    slot = lambda n: (n + 255) // 256 * 256 if n else 256
    arena = sum(slot(n) for n in (80 * len(files), src_end - src_base, 4 * words, dst_end - dst_base, 4 * strips, 4 * len(files)))
    return (src_base, src_end - src_base, dst_base, dst_end - dst_base, words, strips, rowsum, int(u8), int(u16), arena), rows


def _layout_cases():
    many = []
    src = dst = 3
    for k in range(65):                                          # 65 files, every seventh left out, 16-bit ones on even offsets
        bps = 2 if k % 5 == 0 else 1
        dst += dst % 2 if bps == 2 else 0
        H, W, rps = 1 + k % 7, 1 + k % 11, 1 + k % 3
        many.append(_f(src, 100 + k, dst, H, W, spp=1 + k % 4, bps=bps, rps=rps, predictor=k % 2, swap=k % 3 == 0, lzw=k % 4 != 0, in_batch=k % 7 != 6))
        src += 100 + k + (k % 3)
        dst += H * W * (1 + k % 4) * bps + (k % 4)
    return [
        [_f(0, 500, 0, 5, 7)],                                                                   # one file
        [_f(10, 500, 6, 5, 7, spp=3, rps=2), _f(600, 80, 300, 3, 65, bps=2, swap=1)],             # two, gaps in both buffers
        [_f(0, 50, 0, 3, 5), _f(50, 60, 15, 2, 2, bps=2, predictor=1)],                           # an odd raster end before a 16-bit file: refused
        [_f(0, 50, 0, 3, 5), _f(50, 60, 16, 2, 2, bps=2, predictor=1)],                           # the same one byte on
        [_f(0, 50, 1, 3, 5, predictor=1), _f(50, 60, 20, 2, 2, bps=2)],                           # an odd base: the 16-bit offset stays even from dst_base
        [_f(0, 50, 0, 3, 5, in_batch=0), _f(50, 60, 16, 41, 43, rps=41), _f(200, 10, 0, 1, 1, in_batch=0)],   # zero-strip files first and last
        [_f(0, 50, 0, 3, 5, in_batch=0)],                                                         # nothing takes part
        [_f(0, 90, 0, 40, 50, rps=10, n_table=2), _f(90, 10, 2000, 1, 1, lzw=0)],                 # a table shorter than the image
        many,
    ]


def test_the_layout_function_equals_its_restatement(layout_exe, tmp_path):
    cases = _layout_cases()
    with open(tmp_path / 'cases.txt', 'w') as f:
        for files in cases:
            for d in files:
                f.write(' '.join(str(int(d[k])) for k in KEYS) + '\n')
            f.write('end\n')
    run = subprocess.run([layout_exe, 'layout', str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    lines = run.stdout.split('\n')
    refused = 0
    for i, files in enumerate(cases):
        want = _restated(files)
        head = lines.pop(0)
        if want is None:
            assert head == 'refused', (i, head)
            refused += 1
            continue
        assert head.split()[0] == 'batch' and tuple(int(v) for v in head.split()[1:]) == want[0], (i, head, want[0])
        for k, row in enumerate(want[1]):
            got = lines.pop(0).split()
            assert got[0] == 'file' and tuple(int(v) for v in got[1:]) == row, (i, k, got, row)
    assert refused == 1 and lines == ['']
    assert len(cases[-1]) == 65 and len(cases[0]) == 1 and len(cases[1]) == 2


# ---- the routing rule for a set of files -----------------------------------------------------------------------------------------
def _file_of_strips(n, compression=5):
    return dc.tiff_file([bytes(2)] * n, n, 8, 1, compression=compression)


def test_the_routing_rule_on_synthetic_file_sets():
    """One rule (csrc/tiff_parse.h, asked through ecseg_tiff_decode_batch_routes by image_io.imread_many): the LZW strips of the
    files ecseg_tiff_decode accepts sum to at least 1040."""
    goes = lambda datas: image_io.tiff_batch_goes_to_device(datas)
    f208, f207 = _file_of_strips(208), _file_of_strips(207)
    assert goes([f208] * 5) == (True, [True] * 5), '5 x 208 = 1040 strips go'
    assert goes([f208] * 4 + [f207])[0] is False, '4 x 208 + 207 do not'
    assert goes([f208] * 4 + [f207, _file_of_strips(1)])[0] is True
    raw, deflate = _file_of_strips(208, compression=1), _file_of_strips(208, compression=8)
    assert goes([f208] * 4 + [raw, deflate]) == (False, [True] * 4 + [False, False]), 'raw and Deflate files do not count'
    assert goes([f208] * 5 + [raw, deflate]) == (True, [True] * 5 + [False, False]), 'and are not sent with a set that goes'
    junk = [b'', b'II*\0', f208[:-20], bytes(100)]
    assert goes([f208] * 4 + junk) == (False, [True] * 4 + [False] * 4), 'unparseable files do not count'
    assert goes([]) == (False, []) and goes([raw]) == (False, [False]), 'an empty set does not go'
    assert goes([_file_of_strips(1040)]) == (True, [True]) and goes([_file_of_strips(1039)])[0] is False
    wide = dc.tiff_file([bytes(2)] * 1040, 1040, 62641, 1)                      # strips of one byte more than any that was measured
    assert goes([wide]) == (False, [False]) and goes([dc.tiff_file([bytes(2)] * 1040, 1040, 62640, 1)]) == (True, [True])
    short = dc.tiff_file([bytes(2)] * 1040, 1040, 8, 1, counts=[2] * 1039)
    assert goes([short]) == (False, [False]), 'a strip table shorter than the image stays on the host, as in the single-file rule'
    behind = dc.offset_behind_the_file()
    assert goes([behind]) == (False, [False]), 'a file ecseg_tiff_decode refuses'
    # the C entry itself on bad arguments: 0
    lib = _lib.load_library()
    buf = np.frombuffer(f208, np.uint8)
    tab = np.array([[0, buf.size + 1]], np.int64)
    assert lib.ecseg_tiff_decode_batch_routes(buf.ctypes.data, buf.size, tab.ctypes.data, 1, 0) == 0
    assert lib.ecseg_tiff_decode_batch_routes(buf.ctypes.data, buf.size, tab.ctypes.data, 0, 0) == 0
    assert lib.ecseg_tiff_decode_batch_bytes(buf.ctypes.data, buf.size, tab.ctypes.data, 1, 0) == -1
    assert lib.ecseg_tiff_decode_batch_bytes(buf.ctypes.data, buf.size, tab.ctypes.data, 0, 0) == 0
    tab[0, 1] = buf.size
    assert lib.ecseg_tiff_decode_batch_bytes(buf.ctypes.data, buf.size, tab.ctypes.data, 1, 0) >= buf.size + 208 * 8


def test_file_images_that_lie_in_one_buffer_are_packed_without_a_copy():
    pool = np.arange(100, dtype=np.uint8)
    views = [pool[3:10], pool[10:40], pool[55:100].reshape(-1)]
    buf, ranges = _lib.pack_file_images(views)
    assert buf is pool and ranges.tolist() == [[3, 7], [10, 30], [55, 45]] and ranges.dtype == np.int64
    for arrs in (views[::-1], [pool[3:10], pool[8:20]], [pool[3:10], np.arange(5, dtype=np.uint8)], [np.frombuffer(b'abc', np.uint8)] * 2):
        buf, ranges = _lib.pack_file_images(arrs)               # out of order, overlapping, of two buffers, of no array: copied
        assert buf is not pool and buf.tobytes() == b''.join(a.tobytes() for a in arrs)
        assert ranges.tolist() == [[sum(a.size for a in arrs[:k]), arrs[k].size] for k in range(len(arrs))]
    buf, ranges = _lib.pack_file_images([])
    assert buf.size == 0 and ranges.shape == (0, 2)


# ---- imread_many -------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _paths(tmp_path):
    rng = np.random.default_rng(5)
    out = []
    for k in range(5):                                           # five LZW files of 208 one-row strips: a set that goes
        p = str(tmp_path / ('lzw_%d.tif' % k))
        open(p, 'wb').write(dc.tiff_file([dc.pack(dc.lzw_codes(rng.integers(0, 9, 8, dtype=np.uint8).tobytes())) for _ in range(208)], 208, 8, 1))
        out.append(p)
    small = str(tmp_path / 'small.tiff')
    image_io.write_tiff_gray8(small, rng.integers(0, 255, (5, 7), dtype=np.uint8))
    npy = str(tmp_path / 'a.npy')
    np.save(npy, rng.integers(0, 255, (4, 4, 3), dtype=np.uint8))
    broken = str(tmp_path / 'broken.tif')
    open(broken, 'wb').write(b'II*\0 not a tiff')
    raw = str(tmp_path / 'raw.tif')
    open(raw, 'wb').write(dc.tiff_file([bytes(range(12))], 3, 4, 3, compression=1))
    return out + [small, npy, broken, str(tmp_path / 'missing.tif'), raw]


def _per_path(paths):
    want = []
    for p in paths:
        try:
            want.append(image_io.imread(p))
        except Exception as e:
            want.append(e)
    return want


def _check_against_imread(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, Exception):
            assert type(g) is type(w) and str(g) == str(w), (g, w)
        else:
            assert _same(g, w)


def test_imread_many_without_a_handle_and_on_handles_that_answer_none_errors_and_arrays(tmp_path):
    paths = _paths(tmp_path)
    want = _per_path(paths)
    assert sum(isinstance(w, Exception) for w in want) == 2
    _check_against_imread(image_io.imread_many(paths), want)
    _check_against_imread(image_io.imread_many(paths, handle=object()), want)         # a handle without the method
    assert image_io.imread_many([]) == []

    class Device:
        def __init__(self, answer):
            self.answer, self.calls = answer, []

        def tiff_decode_many(self, datas):
            self.calls.append([len(d) for d in datas])
            return [self.answer(k, d) for k, d in enumerate(datas)]
    marked = np.full((208, 8), 77, np.uint8)
    err = _lib.EcsegError('ecseg_tiff_decode failed (-1)')
    err.code = -1
    for answer in (lambda k, d: None, lambda k, d: err, lambda k, d: ValueError('x')):
        dev = Device(answer)
        _check_against_imread(image_io.imread_many(paths, handle=dev), want)
        assert dev.calls == [[os.path.getsize(p) for p in paths[:5]] + [os.path.getsize(paths[5])]], 'one call with the LZW files, the small one too'
    dev = Device(lambda k, d: marked if k in (1, 3) else None)                      # an array is taken as it is, in its file's place
    got = image_io.imread_many(paths, handle=dev)
    for k, (g, w) in enumerate(zip(got, want)):
        if k in (1, 3):
            assert g is marked
        elif not isinstance(w, Exception):
            assert _same(g, w)
    dev = Device(lambda k, d: marked)
    image_io.imread_many(paths[3:], handle=dev)                                     # 2 x 208 + 5 strips: the set stays on the host
    assert dev.calls == []


# ---- make stat_fish with tiff_read_batch ---------------------------------------------------------------------------------------
class ManyReadingHandle(cpu.RenderingOracleHandle):
    """A handle whose ``tiff_decode`` and ``tiff_decode_many`` are answered by the host reader and recorded."""

    def _host(self, data):
        path = os.path.join(self.tmp, 'decode.tif')
        with open(path, 'wb') as f:
            f.write(data)
        try:
            return image_io.read_tiff(path)
        except Exception:
            e = _lib.EcsegError('ecseg_tiff_decode failed (-1)')
            e.code = -1
            return e

    def tiff_decode(self, data):
        self.calls.append(dict(tiff_decode=len(data)))
        a = self._host(data)
        if isinstance(a, Exception):
            raise a
        return a

    def tiff_decode_many(self, datas):
        self.calls.append(dict(tiff_decode_many=len(datas)))
        return [self._host(d) for d in datas]


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


def test_tiff_read_batch_3_over_seven_images_writes_what_1_writes(tmp_path, monkeypatch, capsys):
    """Seven small images, one file corrupt and one mask missing; every set is sent (the rule is replaced, to see the calls)."""
    inp, _ = cpu.make_folder(tmp_path, kinds=(('img_0', 'tif'), ('img_1', 'tif'), ('img_6', 'npy8')), size=(40, 50))
    for k in (2, 3, 4, 5):                                        # the folder's scenes again under further names
        shutil.copyfile(inp / ('img_%d.tif' % (k % 2)), inp / ('img_%d.tif' % k))
        shutil.copyfile(inp / 'nuclei_masks' / ('img_%d.tif' % (k % 2)), inp / 'nuclei_masks' / ('img_%d.tif' % k))
    data = bytearray(open(inp / 'img_2.tif', 'rb').read())
    data[len(data) // 2:len(data) // 2 + 40] = bytes(40)         # the strips' streams are damaged
    data[8:60] = b'\xff' * 52
    open(inp / 'img_2.tif', 'wb').write(bytes(data))
    os.remove(inp / 'nuclei_masks' / 'img_4.tif')
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data: True)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', lambda datas: (True, [True] * len(datas)))
    runs = {}
    for k in (1, 3):
        _set_key(tmp_path, tiff_read_on_device=True, tiff_read_batch=k)
        handle = ManyReadingHandle()
        handle.tmp = str(tmp_path)
        with pytest.raises(SystemExit) as e:
            sf.main([], handle=handle)
        runs[k] = (cpu.folder_bytes(inp / 'annotated'), e.value.code, capsys.readouterr().out, handle.calls)
        shutil.rmtree(inp / 'annotated')
    assert runs[1][1] == runs[3][1] == 1
    assert runs[1][2] == runs[3][2], 'the messages differ'
    assert 'img_2.tif - cannot be read' in runs[1][2] and 'img_4.tif - has no nucleus mask' in runs[1][2]
    assert sorted(runs[1][0]) == sorted(runs[3][0]) and len(runs[1][0]) > 5 * 5
    for f in runs[1][0]:
        assert runs[1][0][f] == runs[3][0][f], f
    assert not [c for c in runs[1][3] if 'tiff_decode_many' in c]
    many = [c['tiff_decode_many'] for c in runs[3][3] if 'tiff_decode_many' in c]
    assert many == [6, 5, 1], 'three chunks: 3 images + 3 masks, 3 images + 2 masks, and the mask of the .npy image'
    # the key is ignored without tiff_read_on_device
    _set_key(tmp_path, tiff_read_on_device=False, tiff_read_batch=3)
    handle = ManyReadingHandle()
    handle.tmp = str(tmp_path)
    with pytest.raises(SystemExit):
        sf.main([], handle=handle)
    assert not [c for c in handle.calls if 'tiff_decode' in c or 'tiff_decode_many' in c]
    got = cpu.folder_bytes(inp / 'annotated')
    assert sorted(got) == sorted(runs[1][0]) and all(got[f] == runs[1][0][f] for f in got)


@pytest.mark.parametrize('value', [0, -2, True, 'four', 2.0, [3], None])
def test_a_tiff_read_batch_that_is_no_positive_integer_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_read_batch=value)
    monkeypatch.chdir(tmp_path)
    handle = ManyReadingHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'tiff_read_batch must be a positive integer' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not [d for d in os.listdir(inp) if d.startswith('tmp_')] and not handle.calls


def test_a_handle_without_tiff_decode_many_is_a_configuration_error_above_1(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    monkeypatch.chdir(tmp_path)

    del_many = type('NoMany', (cpu.RenderingOracleHandle,), {'tiff_decode': ManyReadingHandle.tiff_decode, '_host': ManyReadingHandle._host})
    _set_key(tmp_path, tiff_read_on_device=True, tiff_read_batch=2)
    handle = del_many()
    handle.tmp = str(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    out = capsys.readouterr().out
    assert e.value.code == 2 and 'tiff_read_batch: 2 needs the batched device TIFF reader (tiff_decode_many)' in out and not handle.calls
    _set_key(tmp_path, tiff_read_on_device=True, tiff_read_batch=1)          # the same handle runs one by one
    sf.main([], handle=handle)
    assert os.path.isdir(inp / 'annotated')
