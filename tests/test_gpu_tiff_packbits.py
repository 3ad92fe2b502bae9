"""PackBits TIFF files (compression 32773) decoded on the device behind the handle option ``tiff_packbits_on_device``
(tiffb_packbits_kernel, csrc/tiff_packbits_strip.h): every file of tiff_packbits_cases.py through ``Handle.tiff_decode`` and
``Handle.tiff_decode_many`` equals ``image_io.read_tiff``'s samples, strips and tiles; the streams built by hand have the Python
decoder's verdict - it raises for no stream, so each is status 0 with its bytes, the strip one byte short included (the missing
sample is zero, as in the Python reader); a batch that mixes the four kinds of file gives each its own lone decode; and a handle with
the option off answers -5 (None) as before."""
import contextlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_decode_cases as dc               # noqa: E402
import tiff_packbits_cases as pc             # noqa: E402
import tiff_tiles_cases as tc                # noqa: E402
from ecseg_amd._lib import E_UNSUPPORTED, pack_file_images      # noqa: E402

pytestmark = pytest.mark.gpu
OPTIONS = ('tiff_deflate_on_device', 'tiff_tiled_on_device', 'tiff_packbits_on_device')


@contextlib.contextmanager
def options(h, **on):
    """The named handle options on for the block, every one of the three off behind it (the session's handle goes back as it came)."""
    try:
        h.set_option('tiff_deflate_on_device', int(bool(on.get('deflate'))))
        h.set_option('tiff_tiled_on_device', int(bool(on.get('tiled'))))
        h.set_option('tiff_packbits_on_device', int(bool(on.get('packbits'))))
        yield h
    finally:
        for key in OPTIONS:
            h.set_option(key, 0)


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    """(name, the Python reader's samples, file bytes, tiled) of every plan, read once"""
    tmp = tmp_path_factory.mktemp('packbits')
    return [(name, pc.python_read(data, tmp), data, tiled) for name, _, data, tiled in pc.plan_cases()]


@pytest.fixture(scope='module')
def hand(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('packbits_hand')
    return [(name, pc.python_read(data, tmp), data) for name, _, data in pc.hand_cases()]


def test_a_default_handle_leaves_every_packbits_file_to_the_python_reader(gpu, cases):
    """The control: nothing changes with the option off - None (ECSEG_E_UNSUPPORTED) from both calls, strips and tiles, -5 without a shape."""
    with options(gpu):
        name, ref, data, _ = cases[0]
        assert gpu.tiff_decode(data) is None
        assert gpu.tiff_decode_many([d for _, _, d, _ in cases]) == [None] * len(cases)
        shapes, status = gpu.tiff_decode_packed(*pack_file_images([np.frombuffer(data, np.uint8)]))
        assert status.tolist() == [E_UNSUPPORTED] and shapes.tolist() == [[0, 0, 0, 0]]
    with options(gpu, tiled=True, deflate=True):             # the other two options do not take them either
        assert gpu.tiff_decode_many([d for _, _, d, _ in cases]) == [None] * len(cases)


def test_every_plan_decodes_to_the_python_readers_samples_alone(gpu, cases):
    with options(gpu, packbits=True, tiled=True):
        for name, ref, data, tiled in cases:
            got = gpu.tiff_decode(data)
            assert got is not None and got.dtype == ref.dtype and np.array_equal(got, ref), name
    with options(gpu, packbits=True):                        # tiles need their own option on top
        for name, ref, data, tiled in cases:
            got = gpu.tiff_decode(data)
            assert (got is None) if tiled else np.array_equal(got, ref), name


def test_every_plan_decodes_to_the_python_readers_samples_in_one_batch(gpu, cases):
    with options(gpu, packbits=True, tiled=True):
        many = gpu.tiff_decode_many([d for _, _, d, _ in cases])
    for (name, ref, _, _), got in zip(cases, many):
        assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and np.array_equal(got, ref), name


def test_the_streams_built_by_hand_have_the_python_decoders_verdict(gpu, hand):
    """Status 0 and the Python reader's samples for each: image_io._packbits_decode raises for no stream (tests/test_tiff_packbits.py), so
    the strip whose stream is one byte short is read with its missing byte zero, and trailing bytes are not looked at."""
    assert pc.RAISING_STREAMS == []
    with options(gpu, packbits=True):
        many = gpu.tiff_decode_many([d for _, _, d in hand])
        for (name, ref, data), got in zip(hand, many):
            assert isinstance(got, np.ndarray) and np.array_equal(got, ref), name
            assert np.array_equal(gpu.tiff_decode(data), ref), name
        datas = [np.frombuffer(d, np.uint8) for _, _, d in hand]
        _, status = gpu.tiff_decode_packed(*pack_file_images(datas))
        assert status.tolist() == [0] * len(hand)
    short = dict((n, r) for n, r, _ in hand)['stream_one_byte_short']
    assert (short[2:4].reshape(-1)[-1] == 0), 'the byte the stream does not give is zero'


def test_a_stream_longer_than_the_staged_bytes_and_a_strip_table_shorter_than_the_image(gpu, tmp_path):
    """Noise in one strip of 9 x 700 bytes (all literals: the stream passes the 1024 bytes staged in LDS several times, and headers fall
    on every position of the staged bytes), and a file whose tables have fewer strips than the image: the rest is zeros."""
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (9, 700), dtype=np.uint8)
    mixed = noise.copy()
    mixed[:, 100:450] = 3                                    # runs of 128, 128, 94 between literals
    img = tc.squeeze(tc.pixels('gray8', 33, 70))
    streams = [pc.packbits(s) for s in pc.raw_strips(img, 5)]
    files = [pc.strip_file(noise, 9, min_run=200), pc.strip_file(mixed, 9), pc.strip_file(img, 5, streams=streams[:4])]
    refs = [pc.python_read(d, tmp_path) for d in files]
    assert np.array_equal(refs[0], noise) and np.array_equal(refs[1], mixed) and not refs[2][20:].any() and np.array_equal(refs[2][:20], img[:20])
    with options(gpu, packbits=True):
        for ref, data, got in zip(refs, files, gpu.tiff_decode_many(files)):
            assert np.array_equal(got, ref) and np.array_equal(gpu.tiff_decode(data), ref)


def test_a_batch_that_mixes_the_four_kinds_gives_each_file_its_lone_decode(gpu, cases, tmp_path):
    img8, img16 = tc.pixels('rgb8', 40, 70), tc.pixels('rgb16', 40, 70)
    rows = img8.reshape(40, -1)
    by_name = dict((n, d) for n, _, d, _ in cases)
    files = [dc.file_of(img8, 5, predictor=2),                                                           # LZW strips
             by_name['rgb16_40x70_rps5_p2_be'],                                                          # PackBits strips
             dc.tiff_file([zlib.compress(rows[r:r + 7].tobytes()) for r in range(0, 40, 7)], 40, 70, 7, spp=3, compression=8),   # Deflate strips
             tc.tiled_tiff(img16, 16, 16, 5, 2, '>'),                                                    # LZW tiles
             by_name['rgb8_40x70_t16x16_p2_le'],                                                         # PackBits tiles
             tc.tiled_tiff(img8, 16, 32, 8, 1, '<'),                                                     # Deflate tiles
             dc.file_of(img8, 40, compression=1),                                                        # uncompressed
             by_name['gray8_33x70_rps1_p1_le']]
    refs = [pc.python_read(d, tmp_path) for d in files]
    with options(gpu, packbits=True, tiled=True, deflate=True):
        many = gpu.tiff_decode_many(files)
        for k, (ref, data, got) in enumerate(zip(refs, files, many)):
            assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and np.array_equal(got, ref), k
            assert np.array_equal(gpu.tiff_decode(data), got), k
