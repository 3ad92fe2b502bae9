"""PackBits TIFF files (compression 32773) for the tests of the device reader's PackBits path (test_tiff_packbits.py,
test_gpu_tiff_packbits.py, test_gpu_metaseg_tiff_kinds.py): a small PackBits encoder, the one new writer - the files around its
streams are tiff_decode_cases.tiff_file's (strips) and tiff_tiles_cases.tiled_tiff's (tiles) -, the shapes and plans both test files
walk, and the streams built by hand.

The oracle of all of them is ``image_io.read_tiff`` with ``image_io._packbits_decode``, which raises for no stream: one that ends
early gives what it has and zeros behind, a run that passes the strip's end is cut, bytes left over are not looked at.  So
``RAISING_STREAMS`` is empty, and every hand stream has status 0 and the Python reader's samples."""
import numpy as np

import tiff_decode_cases as dc
import tiff_tiles_cases as tc

PACKBITS = 32773


def packbits(raw, min_run=3, noop_every=0):
    """bytes -> a PackBits stream: runs of ``min_run`` or more equal bytes as repeats (at most 128), the rest as literal runs (at most
    128); ``noop_every``: a 0x80 header in front of every so-many-th run."""
    raw, out, i, runs = bytes(raw), bytearray(), 0, 0
    n = len(raw)
    while i < n:
        runs += 1
        if noop_every and runs % noop_every == 0:
            out.append(0x80)
        r = 1
        while i + r < n and r < 128 and raw[i + r] == raw[i]:
            r += 1
        if r >= min_run:
            out += bytes([257 - r, raw[i]])
            i += r
            continue
        j = i
        while j < n and j - i < 128:
            r = 1
            while j + r < n and r < min_run and raw[j + r] == raw[j]:
                r += 1
            if r >= min_run:
                break
            j += 1
        j = max(j, i + 1)
        out += bytes([j - i - 1]) + raw[i:j]
        i = j
    return bytes(out)


def raw_strips(img, rps, predictor=1, big_endian=False):
    """The strips of (H, W[, C]) samples as the file holds them before compression (tiff_decode_cases.file_of's steps)."""
    H, W = img.shape[:2]
    a = img.reshape(H, W, -1)
    if predictor == 2:
        d = a.copy()
        d[:, 1:] = a[:, 1:] - a[:, :-1]
        a = d
    if a.dtype == np.uint16:
        a = a.astype('>u2' if big_endian else '<u2')
    rows = a.reshape(H, -1)
    return [rows[r:r + rps].tobytes() for r in range(0, H, rps)]


def strip_file(img, rps, predictor=1, big_endian=False, streams=None, **enc):
    """A PackBits file of strips around ``img``; ``streams``: the strips' bytes instead of the encoder's own."""
    H, W = img.shape[:2]
    spp = 1 if img.ndim == 2 else img.shape[2]
    if streams is None:
        streams = [packbits(s, **enc) for s in raw_strips(img, rps, predictor, big_endian)]
    return dc.tiff_file(streams, H, W, rps, spp=spp, bits=8 * img.dtype.itemsize, compression=PACKBITS, predictor=predictor, big_endian=big_endian)


def tile_file(img, th, tw, predictor=1, big_endian=False, **enc):
    """A PackBits file of tiles around ``img`` (edge tiles padded with 0xA5 bytes, as tiff_tiles_cases writes them)."""
    a = img if img.ndim == 3 else img[..., None]
    bo = '>' if big_endian else '<'
    streams = [packbits(t, **enc) for t in tc.tile_streams(a, th, tw, 1, predictor, bo)]
    return tc.tiled_tiff(a, th, tw, PACKBITS, predictor, bo, streams=streams)


# ---- the shapes and plans ---------------------------------------------------------------------------------------------------------------
def images():
    """name -> samples: gray8 33 x 70, RGB8 96 x 128, RGB16 40 x 70 (the latter also the image of the 16 x 16 tiles with padded edges)"""
    return {'gray8_33x70': tc.squeeze(tc.pixels('gray8', 33, 70)), 'rgb8_96x128': tc.pixels('rgb8', 96, 128), 'rgb16_40x70': tc.pixels('rgb16', 40, 70),
            'gray8_40x70': tc.squeeze(tc.pixels('gray8', 40, 70)), 'rgb8_40x70': tc.pixels('rgb8', 40, 70)}


def plan_cases():
    """[(name, samples as read_tiff returns them, file bytes, tiled)]: every shape at 1, 5 and all rows per strip; RGB16 in both byte
    orders with and without predictor 2; 8-bit predictor 2; tiles of 16 x 16 on the 40 x 70 images, whose edge tiles are padded."""
    im, out = images(), []
    for name in ('gray8_33x70', 'rgb8_96x128', 'rgb16_40x70'):
        img = im[name]
        for rps in (1, 5, img.shape[0]):
            variants = [(p, be) for p in (1, 2) for be in (False, True)] if img.dtype == np.uint16 else [(1, False), (2, False)]
            for pred, be in variants:
                out.append(('%s_rps%d_p%d_%s' % (name, rps, pred, 'be' if be else 'le'), img, strip_file(img, rps, pred, be, noop_every=5 if rps == 5 else 0), False))
    for name in ('gray8_40x70', 'rgb8_40x70', 'rgb16_40x70'):
        img = im[name]
        variants = [(p, be) for p in (1, 2) for be in (False, True)] if img.dtype == np.uint16 else [(1, False), (2, False)]
        for pred, be in variants:
            out.append(('%s_t16x16_p%d_%s' % (name, pred, 'be' if be else 'le'), img, tile_file(img, 16, 16, pred, be), True))
    return out


# ---- streams built by hand ------------------------------------------------------------------------------------------------------------
RAISING_STREAMS = []     # (name, stream, expected, reason): the streams for which image_io._packbits_decode raises - it raises for none


def hand_cases():
    """[(name, samples the Python reader returns, file bytes)]: gray files of 200 pixels per row whose strips are written by hand."""
    rng = np.random.default_rng(32773)
    out = []
    W = 200
    lit = rng.integers(0, 256, 128, dtype=np.uint8)
    row = np.concatenate([lit, np.full(W - 128, 9, np.uint8)])
    out.append(('literal_run_of_128', row[None], strip_file(row[None], 1, streams=[bytes([127]) + lit.tobytes() + bytes([257 - (W - 128), 9])])))
    row = np.concatenate([np.full(128, 200, np.uint8), np.arange(W - 128, dtype=np.uint8)])
    out.append(('repeat_run_of_128', row[None], strip_file(row[None], 1, streams=[bytes([257 - 128, 200, W - 128 - 1]) + row[128:].tobytes()])))
    two = np.concatenate([np.full(150, 1, np.uint8), np.full(100, 7, np.uint8), np.full(150, 3, np.uint8)]).reshape(2, W)
    s = bytes([257 - 128, 1, 257 - 22, 1, 257 - 100, 7, 257 - 128, 3, 257 - 22, 3])          # the run of 100 sevens crosses the row end
    out.append(('run_crosses_a_row_end', two, strip_file(two, 2, streams=[s])))
    row = np.concatenate([np.full(100, 5, np.uint8), np.arange(100, dtype=np.uint8)])
    out.append(('noop_between_runs', row[None], strip_file(row[None], 1, streams=[bytes([0x80, 257 - 100, 5, 0x80, 0x80, 99]) + row[100:].tobytes() + b'\x80'])))
    flat = np.full((7, W), 77, np.uint8)
    out.append(('one_value_all_repeats', flat, strip_file(flat, 3)))
    noise = rng.integers(0, 256, (9, W), dtype=np.uint8)
    data = strip_file(noise, 4, min_run=200)
    assert len(data) > noise.size                          # all literals: the stream is longer than the raster
    out.append(('noise_all_literals', noise, data))
    # a strip whose stream is one byte short: the Python reader takes what there is and zero-fills (it raises for no stream)
    img = rng.integers(0, 256, (6, W), dtype=np.uint8)
    img[:, 50:120] = 31
    streams = [packbits(s) for s in raw_strips(img, 2)]
    streams[1] = streams[1][:-1]
    out.append(('stream_one_byte_short', None, strip_file(img, 2, streams=streams)))
    cut = [packbits(s) for s in raw_strips(img, 2)]
    cut[2] = cut[2][:len(cut[2]) // 2]
    out.append(('stream_cut_in_half', None, strip_file(img, 2, streams=cut)))
    lone = [packbits(s) for s in raw_strips(img, 2)]
    lone[2] = bytes([257 - 128])                           # a repeat header that is the stream's last byte: nothing
    out.append(('lone_repeat_header', None, strip_file(img, 2, streams=lone)))
    # bytes left over behind the strip's last byte are not looked at
    trail = [packbits(s) + bytes([0x7f, 1, 2, 3, 0x90]) for s in raw_strips(img, 2)]
    out.append(('trailing_bytes', img, strip_file(img, 2, streams=trail)))
    # a run that would pass the strip's end is cut there
    over = [packbits(s) for s in raw_strips(img, 2)]
    over[0] = packbits(raw_strips(img, 2)[0][:-3]) + bytes([257 - 100, img[1, -3]])
    ref = img.copy()
    ref[1, -3:] = img[1, -3]
    out.append(('run_passes_the_strip_end', ref, strip_file(img, 2, streams=over)))
    return out


def python_read(data, tmp_path, name='case'):
    """image_io.read_tiff's samples of the file (the Python reader: the native one leaves PackBits to it)."""
    import os

    from ecseg_amd import image_io
    path = os.path.join(str(tmp_path), name + '.tif')
    with open(path, 'wb') as f:
        f.write(data)
    return image_io.read_tiff(path)
