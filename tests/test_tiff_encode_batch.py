"""The batched device TIFF encoder without a GPU: the new symbols, the layout function against a restatement, the case list of
tests/tiff_encode_batch_cases.py against the host writers and held to the branches it is named for, the layout and the strip routine
of the encode kernels compiled for the host under ASan + UBSan (tools/asan/tiff_encode_batch_fuzz.cpp), and the ``tiff_write_batch``
key of ``make stat_fish`` on injected handles."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lzw_ref                               # noqa: E402
import test_stat_fish_aqua as cpu            # noqa: E402
import test_tiff_encode as te                # noqa: E402
import tiff_encode_batch_cases as bc         # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENCODED = {}


def encoded(case):
    """The restatement's strips of a case, computed once for the tests that need them."""
    if case.name not in _ENCODED:
        _ENCODED[case.name] = [lzw_ref.encode(s) for s in lzw_ref.strips(case.img, case.invert)]
    return _ENCODED[case.name]


def test_header_binding_and_documents_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert ('int ecseg_tiff_encode_batch(ecseg_ctx* h, const uint8_t* rasters, long long raster_bytes, const int64_t* files /* [n][5] offset, H, W, spp, invert */,\n'
            '                            int n_files, uint8_t* out, long long out_cap, int64_t* out_ranges /* [n][2] offset, n_bytes */);') in hdr
    assert 'long long ecseg_tiff_encode_batch_bytes(const int64_t* files, int n_files);' in hdr
    assert 'int ecseg_fish_render_tiff_batch(ecseg_ctx* h, int n_images, const uint8_t* const* imgs, const int32_t* shapes' in hdr
    assert 'still 5 - additive: ecseg_tiff_encode_batch' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'still 5 - additive: ecseg_tiff_encode_bound' in hdr                 # the earlier lines stay
    lib = _lib.load_library()
    for name in ('ecseg_tiff_encode_batch', 'ecseg_tiff_encode_batch_bytes', 'ecseg_fish_render_tiff_batch'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(_lib.Handle, 'tiff_encode_many') and hasattr(_lib.Handle, 'fish_render_tiff_many') and hasattr(_lib.Handle, 'tiff_encode_packed')
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_write_batch' in text and 'ecseg_tiff_encode_batch' in text, doc
    assert 'asan_tiff_encode_batch:' in open(os.path.join(ROOT, 'Makefile')).read()
    kernels = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_kernels.hip')).read()
    for k in ('tiffb_lzw_strip_kernel', 'tiffb_scan_kernel', 'tiffb_place_kernel', 'tiffb_gather_kernel', 'tl_strip('):
        assert k in kernels, k
    assert 'static_assert(sizeof(TeFile) == 72' in open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_encode_batch.h')).read()
    assert '# tiff_write_batch' in open(os.path.join(ROOT, 'config.yaml')).read()
    assert 'tiff_write_batch' not in (yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish'])


def test_the_sizing_entry_point_refuses_what_the_call_refuses():
    lib = _lib.load_library()
    size = lambda rows: lib.ecseg_tiff_encode_batch_bytes(np.array(rows, np.int64).ctypes.data, len(rows))
    assert lib.ecseg_tiff_encode_batch_bytes(None, 0) == 0 and lib.ecseg_tiff_encode_batch_bytes(None, 1) == -1
    assert size([[0, 5, 7, 1, 0]]) >= 72 + 35 + 2 * 35 + 64
    for bad in ([0, 0, 7, 1, 0], [0, 5, 0, 1, 0], [0, 5, 7, 2, 0], [0, 5, 7, 4, 0], [0, -1, 7, 1, 0], [0, 1, 1 << 30, 1, 0], [0, 1 << 40, 1, 1, 0]):
        assert size([bad]) == -1 and size([[0, 5, 7, 1, 0], [35] + bad[1:]]) == -1, bad
    assert size([[0, 5, 7, 1, 0], [34, 5, 7, 3, 1]]) == -1, 'a raster that starts inside the one in front'
    assert size([[3, 5, 7, 1, 0], [100, 5, 7, 3, 1]]) > 0, 'gaps are allowed'
    assert lib.ecseg_tiff_encode_batch_bytes(np.zeros((65536, 5), np.int64).ctypes.data, 65536) == -1


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------
def _build_fuzz(tmp, cxx, san):
    exe = str(tmp / ('tiff_encode_batch_fuzz' + ('_san' if san else '')))
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(ROOT, 'ecseg_amd', 'csrc', 'host_codec.cpp'), os.path.join(ROOT, 'tools', 'asan', 'tiff_encode_batch_fuzz.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope='module')
def fuzz_builds(tmp_path_factory):
    """(the program built with the sanitizers, or None where the host compiler cannot link their runtimes; a plain build then)."""
    tmp = tmp_path_factory.mktemp('encode_batch_fuzz')
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp / 'probe')], capture_output=True, timeout=120).returncode != 0:
        return None, _build_fuzz(tmp, cxx, [])
    return _build_fuzz(tmp, cxx, san), None


def test_layout_and_strip_routine_run_clean_under_the_sanitizers(fuzz_builds):
    """The stand-alone program (its own main, no preloaded runtime), -Wall -Werror: seeded file lists through the layout, their strips
    and the built-in strips through the routine of the kernels, against the host encoder."""
    if fuzz_builds[0] is None:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    run = subprocess.run([fuzz_builds[0]], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_encode_batch_fuzz ok' in run.stdout and ' 0 strips encoded' not in run.stdout, run.stdout


def test_make_asan_tiff_encode_batch_builds_and_runs_clean():
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    out = subprocess.run(['make', '-C', ROOT, 'asan_tiff_encode_batch'], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0 and 'tiff_encode_batch_fuzz ok' in out.stdout, (out.stdout + out.stderr)[-3000:]


# ---- the layout function against a restatement ----------------------------------------------------------------------------------
def _restated(files):
    """What te_batch_layout and tiff_encode_batch_bufs give, from their description alone.  files: (src_off, H, W, spp, invert).  Strips of
    max(1, min(H, 8192 // line)) rows; a slot is 2 * strip bytes + 64 rounded up to 16; a file's frame is 8 + 150 bytes, + 8 per strip with
    more than one, + 6 with three samples; everything else is a running sum; the arena holds seven slots on multiples of 256 bytes."""
    if len(files) > 65535:
        return None
    base = min([f[0] for f in files], default=0)
    end = max([f[0] + f[1] * f[2] * f[3] for f in files], default=0)
    rows, strips, slots, offs, packed, most = [], 0, 0, 0, 0, 0
    for off, H, W, spp, invert in files:
        line = W * spp
        rps = max(1, min(H, 8192 // line))
        ns = -(-H // rps)
        stride = (2 * rps * line + 64 + 15) // 16 * 16
        frame = 8 + 150 + (8 * ns if ns > 1 else 0) + (6 if spp == 3 else 0)
        rows.append((off - base, slots, stride, offs, frame, rps, 255 if invert else 0, strips, ns))
        strips += ns
        slots += ns * stride
        offs += ns + 1
        packed += frame + ns * stride
        most = max(most, ns)
    slot = lambda n: (n + 255) // 256 * 256 if n else 256
    arena = sum(slot(n) for n in (72 * len(files), end - base, slots, 4 * strips, 8 * offs, 8 * (len(files) + 1), packed))
    return (base, end - base, strips, most, slots, offs, packed, arena), rows


def _layout_cases():
    rng = np.random.default_rng(77)
    many, at = [], 5
    for k in range(40):
        H, W, spp = int(rng.integers(1, 71)), int(rng.integers(1, 71)), 1 + 2 * (k % 2)
        at += int(rng.integers(0, 30)) * (k % 3 == 0)
        many.append((at, H, W, spp, k % 5 == 0))
        at += H * W * spp
    return [
        [],
        [(0, 1, 1, 1, 0)],
        [(7, 7, 1392, 1, 0), (20000, 2, 2731, 3, 1)],                              # a gap, a short last strip, a line above 8192
        [(0, 1040, 1392, 3, 0)] * 0 + [(0, 1040, 1392, 3, 0), (4343040, 1040, 1392, 1, 0)],     # stat_fish's two plans: 1040 and 208 strips
        [tuple(r) for r in bc.pack([bc.CASES[i] for i in bc.BATCHES['17_files']], gaps=[k % 4 for k in range(17)])[1].tolist()],
        many,
        [(i, 1, 1, 1, 0) for i in range(65536)],                                   # refused: grid y is the file
    ]


def test_the_layout_function_equals_its_restatement(fuzz_builds, tmp_path):
    cases = _layout_cases()
    with open(tmp_path / 'cases.txt', 'w') as f:
        for files in cases:
            for d in files:
                f.write(' '.join(str(int(v)) for v in d) + '\n')
            f.write('end\n')
    run = subprocess.run([fuzz_builds[0] or fuzz_builds[1], 'layout', str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=120)
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
            assert row[0] % 1 == 0 and row[4] % 2 == 0 and row[2] % 16 == 0, 'frames are even, so every file and strip starts on an even offset'
    assert refused == 1 and lines == ['']
    assert [r[8] for r in _restated(cases[3])[1]] == [1040, 208] and [r[7] for r in _restated(cases[3])[1]] == [0, 1040]


# ---- the case list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', bc.CASES, ids=[c.name for c in bc.CASES])
def test_the_expected_file_is_the_host_writers_and_decodes_back(case, tmp_path):
    want = lzw_ref.tiff_file(case.img, case.invert, encoded(case))
    path = str(tmp_path / 'a.tif')
    if bc.spp(case) == 1:
        image_io.write_tiff_gray8(path, case.img, invert=case.invert)
    else:
        assert not case.invert
        image_io.write_tiff_rgb8(path, case.img)
    assert open(path, 'rb').read() == want
    back = image_io.read_tiff(path)                              # (ecseg_tiff_read)
    assert back.dtype == np.uint8 and np.array_equal(back, ~case.img if case.invert else case.img)


def test_the_case_list_takes_the_branches_it_is_named_for():
    raw = {c.name: lzw_ref.strips(c.img, c.invert) for c in bc.CASES}
    enc = {c.name: encoded(c) for c in bc.CASES}
    case = lambda part: next(c for c in bc.CASES if part in c.name)
    assert {c.img.shape for c in bc.CASES} >= {(1, 1), (1, 1, 3)}
    assert any(c.invert for c in bc.CASES) and any(not c.invert for c in bc.CASES) and {bc.spp(c) for c in bc.CASES} == {1, 3}
    short = raw[case('short_last').name]
    assert [len(s) for s in short] == [5 * 1392, 2 * 1392], 'rows per strip 5, a last strip of 2 rows'
    lengths = {len(s) for name in raw for s in raw[name]}
    assert {bc.CHUNK - 1, bc.CHUNK, bc.CHUNK + 1} <= lengths, 'strips of 1023, 1024 and 1025 staged bytes'
    assert len(raw[case('exactly_a_chunk').name]) == 1 and case('exactly_a_chunk').img.shape[0] == 8, 'the 1024 bytes are several rows'
    wide = raw[case('line_8193').name]
    assert [len(s) for s in wide] == [8193, 8193], 'one row per strip, wider than 8192 bytes'
    inside = case('restart_inside')
    assert len(raw[inside.name]) == 1 and len(raw[inside.name][0]) == 8192 and enc[inside.name][0].restarts >= 1
    assert bc.restart_byte(raw[inside.name][0]) % bc.CHUNK not in (0, bc.CHUNK - 1), 'the restart is inside a chunk'
    border = case('chunk_border')
    assert len(raw[border.name]) == 1 and bc.restart_byte(raw[border.name][0]) % bc.CHUNK == bc.CHUNK - 1, 'the restart eats the last byte of a chunk'
    assert len(raw[border.name][0]) > bc.restart_byte(raw[border.name][0]) + 1, 'and the strip goes on behind it'
    const = case('constant_strip')
    assert len(raw[const.name]) == 1 and len(raw[const.name][0]) == 8192 and len(enc[const.name][0].data) < 300, 'the longest matches'
    every = [e for name in enc for e in enc[name]]
    assert any(e.odd for e in every) and any(not e.odd for e in every), 'strips with and without the pad byte'
    assert any(e.odd for e in enc[case('short_last').name]) and any(not e.odd for e in enc[case('short_last').name]), 'both in one file'
    # the batches: 1 / 2 / 3 / 8 / 17 files in two orders, the large ones with everything
    assert sorted({len(v) for v in bc.BATCHES.values()}) == [1, 2, 3, 8, 17]
    for n in (2, 3, 8, 17):
        a, b = bc.BATCHES['%d_files' % n], bc.BATCHES['%d_files_shuffled' % n]
        assert sorted(a) == sorted(b) and a != b, n
    assert bc.BATCHES['1_files'] != bc.BATCHES['1_files_shuffled']
    for name in ('17_files', '8_files'):
        members = [bc.CASES[i] for i in bc.BATCHES[name]]
        assert {bc.spp(c) for c in members} == {1, 3} and {c.invert for c in members} == {True, False}
    assert set(bc.BATCHES['17_files']) == set(range(len(bc.CASES)))
    buf, tab = bc.pack([bc.CASES[i] for i in bc.BATCHES['3_files']], gaps=[3, 0, 5])
    assert tab[:, 0].tolist() == [3, 3 + bc.CASES[0].img.size, 3 + bc.CASES[0].img.size + bc.CASES[4].img.size + 5] and buf[0] == 0xEE


# ---- make stat_fish with tiff_write_batch ---------------------------------------------------------------------------------------
class BatchOracleHandle(te.TiffOracleHandle):
    """A handle whose batched TIFF calls are answered by the restatements too, and recorded."""
    fail_at = None                               # the index of the fish_render_tiff_many call that is refused

    def tiff_encode_many(self, rasters, inverts=None, budget_bytes=8 << 30):
        self.calls.append(dict(tiff_many=len(rasters)))
        return [lzw_ref.tiff_file(r, bool(v)) for r, v in zip(rasters, inverts or [False] * len(rasters))]

    def fish_render_tiff_many(self, items, budget_bytes=8 << 30):
        n_before = len([c for c in self.calls if 'render_tiff_many' in c])
        self.calls.append(dict(render_tiff_many=len(items)))
        if self.fail_at == n_before:
            e = _lib.EcsegError('ecseg_fish_render_tiff_batch failed (-1)')
            e.code = -1
            raise e
        out = []
        for img, channels, thr, bnd, mask, picture in items:
            rasters = cpu.RenderingOracleHandle.fish_render(self, img, channels, thr, bnd)
            self.calls.pop()                                     # (the render inside is not a call of main's)
            out.append(tuple(lzw_ref.tiff_file(r) for r in rasters) + (None if mask is None else lzw_ref.tiff_file(mask),
                                                                       None if picture is None else lzw_ref.tiff_file(picture)))
        return out


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


def _seven_images(tmp_path):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('img_0', 'tif'), ('img_1', 'tif'), ('img_6', 'npy8')), size=(40, 50))
    for k in (2, 3, 4, 5):                                        # the folder's scenes again under further names
        shutil.copyfile(inp / ('img_%d.tif' % (k % 2)), inp / ('img_%d.tif' % k))
        shutil.copyfile(inp / 'nuclei_masks' / ('img_%d.tif' % (k % 2)), inp / 'nuclei_masks' / ('img_%d.tif' % k))
    return inp


def _run(tmp_path, inp, capsys, handle=None, **keys):
    _set_key(tmp_path, **keys)
    handle = handle or BatchOracleHandle()
    code = 0
    try:
        sf.main([], handle=handle)
    except SystemExit as e:
        code = e.code
    got = cpu.folder_bytes(inp / 'annotated')
    shutil.rmtree(inp / 'annotated')
    return got, code, capsys.readouterr().out, handle.calls


def test_tiff_write_batch_3_over_seven_images_makes_three_calls_and_the_same_folder(tmp_path, monkeypatch, capsys):
    inp = _seven_images(tmp_path)
    monkeypatch.chdir(tmp_path)
    one = _run(tmp_path, inp, capsys, tiff_on_device=True, tiff_write_batch=1)
    three = _run(tmp_path, inp, capsys, tiff_on_device=True, tiff_write_batch=3)
    assert one[1] == three[1] == 0 and one[2] == three[2], 'exit code and messages'
    assert [c['render_tiff_many'] for c in three[3] if 'render_tiff_many' in c] == [3, 3, 1]
    assert not [c for c in three[3] if 'render_tiff' in c or 'tiff' in c or 'tiff_many' in c]
    assert len([c for c in one[3] if 'render_tiff' in c]) == 7 and not [c for c in one[3] if 'render_tiff_many' in c]
    assert sorted(one[0]) == sorted(three[0]) and len(one[0]) == 7 * 5 + 2
    for name in one[0]:
        assert one[0][name] == three[0][name], name
    assert one[0]['stat_fish_lsq.csv'].count(b'\n') > 7
    # the key is ignored without tiff_on_device, and composes with tiff_read_batch
    off = _run(tmp_path, inp, capsys, tiff_on_device=False, tiff_write_batch=3)
    assert not [c for c in off[3] if 'render_tiff_many' in c] and all(off[0][n] == one[0][n] for n in one[0])


def test_one_image_failing_mid_folder_leaves_the_report_the_code_and_the_csv_of_1(tmp_path, monkeypatch, capsys):
    inp = _seven_images(tmp_path)
    os.remove(inp / 'nuclei_masks' / 'img_3.tif')
    monkeypatch.chdir(tmp_path)
    one = _run(tmp_path, inp, capsys, tiff_on_device=True, tiff_write_batch=1)
    three = _run(tmp_path, inp, capsys, tiff_on_device=True, tiff_write_batch=3)
    assert one[1] == three[1] == 1 and one[2] == three[2] and 'img_3.tif - has no nucleus mask' in one[2]
    assert [c['render_tiff_many'] for c in three[3] if 'render_tiff_many' in c] == [3, 3], 'the failed image is in no chunk'
    assert sorted(one[0]) == sorted(three[0]) and len(one[0]) == 6 * 5 + 2 and all(one[0][n] == three[0][n] for n in one[0])


def test_a_refused_chunk_fails_its_images_and_no_others(tmp_path, monkeypatch, capsys):
    inp = _seven_images(tmp_path)
    monkeypatch.chdir(tmp_path)
    good = _run(tmp_path, inp, capsys, tiff_on_device=True, tiff_write_batch=3)
    handle = BatchOracleHandle()
    handle.fail_at = 1                                           # the second chunk: img_3, img_4, img_5
    bad = _run(tmp_path, inp, capsys, handle=handle, tiff_on_device=True, tiff_write_batch=3)
    assert bad[1] == 1 and '3 image(s) were NOT processed' in bad[2]
    for k in (3, 4, 5):
        assert ('img_%d.tif - its TIFF files could not be written' % k) in bad[2]
    csv = lambda run: run[0]['stat_fish_lsq.csv'].decode().split('\n')
    assert csv(bad) == [r for r in csv(good) if not r.startswith(('img_3,', 'img_4,', 'img_5,'))], 'no rows of the chunk, the others in order'
    assert len(csv(bad)) < len(csv(good))
    for name in good[0]:
        if name.endswith('.tif') and not name.startswith(('img_3', 'img_4', 'img_5')):
            assert bad[0][name] == good[0][name], name
        if name.endswith('.tif') and name.startswith(('img_3', 'img_4', 'img_5')):
            assert name not in bad[0], name


@pytest.mark.parametrize('value', [0, -2, True, 'four', 2.0, [3], None])
def test_a_tiff_write_batch_that_is_no_positive_integer_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_write_batch=value)
    monkeypatch.chdir(tmp_path)
    handle = BatchOracleHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'tiff_write_batch must be a positive integer' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not [d for d in os.listdir(inp) if d.startswith('tmp_')] and not handle.calls


def test_a_handle_without_the_two_calls_is_a_configuration_error_above_1(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    monkeypatch.chdir(tmp_path)
    _set_key(tmp_path, tiff_on_device=True, tiff_write_batch=2)
    handle = te.TiffOracleHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    out = capsys.readouterr().out
    assert e.value.code == 2 and 'tiff_write_batch: 2 needs the batched device TIFF encoder (tiff_encode_many, fish_render_tiff_many)' in out
    assert not handle.calls and not os.path.exists(inp / 'annotated')
    _set_key(tmp_path, tiff_on_device=True, tiff_write_batch=1)          # the same handle runs one by one
    sf.main([], handle=handle)
    assert os.path.isdir(inp / 'annotated')
