"""Tiled TIFF files for the tests of the device reader's tiled path (test_tiff_tiles.py, test_gpu_tiff_tiles.py): a small writer of the
project's own - zlib for Deflate, the host LZW encoder for LZW, both byte orders, predictor 1 and 2, edge tiles padded with bytes that
are NOT the image's, so that a reader that keeps padding shows - the extents and variants both files walk, and the damaged files.

The writer was cross-checked once against tifffile 2021.7.2: every file of ``fixture_cases`` and of ``all_cases`` read back with
``tifffile.imread`` equals its pixels, but for the five uncompressed one-tile files with predictor 2 (16 x 16 in a 16 x 16 tile), which
that tifffile version reads as one contiguous block without undoing the predictor.  The files of ``fixture_cases`` are stored under
tests/golden/tiff_tiles/ with their pixels, and test_tiff_tiles.py holds the writer to them byte for byte, so a change to the writer
shows."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiff_tiles')

KINDS = {'gray8': (1, np.uint8), 'rgb8': (3, np.uint8), 'rgba8': (4, np.uint8), 'gray16': (1, np.uint16), 'rgb16': (3, np.uint16)}
# (H, W, TileLength, TileWidth): one whole tile; 1 x 1 in a tile; partial edge tiles on both axes; several tiles, extents that are no
# multiple of 64 pixels; a tile wider and taller than the image
EXTENTS = ((16, 16, 16, 16), (1, 1, 16, 16), (33, 70, 16, 16), (33, 70, 16, 32), (130, 257, 32, 32), (130, 257, 64, 16), (64, 48, 64, 64))
COMPRESSIONS = {'raw': 1, 'lzw': 5, 'deflate': 8}


def pixels(kind, H, W, seed=0):
    """A smooth ramp with noise on top: compresses, and no two neighbouring tiles are alike."""
    spp, dt = KINDS[kind]
    rng = np.random.default_rng(1000 * seed + 7 * H + W + spp)
    top = 255 if dt == np.uint8 else 65535
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing='ij')
    img = (y * 37 + x * 101 + c * 5003) % (top + 1) + rng.integers(0, 4, (H, W, spp))
    return (img % (top + 1)).astype(dt)


def _lzw(raw):
    from ecseg_amd import image_io
    return image_io._lzw_encode(raw)


def tile_streams(img, th, tw, comp, pred, bo):
    """The tiles of (H, W, spp) ``img``, row-major, each as the bytes the file holds; padding pixels are 0xA5 bytes."""
    H, W, spp = img.shape
    out = []
    for ty in range(0, H, th):
        for tx in range(0, W, tw):
            tile = np.full((th, tw, spp), 0xA5 if img.dtype == np.uint8 else 0xA5A5, img.dtype)
            part = img[ty:ty + th, tx:tx + tw]
            tile[:part.shape[0], :part.shape[1]] = part
            if pred == 2:
                d = tile.copy()
                d[:, 1:] = tile[:, 1:] - tile[:, :-1]          # (wraps modulo 2^bits)
                tile = d
            raw = tile.astype(tile.dtype.newbyteorder(bo)).tobytes()
            out.append(raw if comp == 1 else _lzw(raw) if comp == 5 else zlib.compress(raw, 6))
    return out


def tiled_tiff(img, th, tw, comp=1, pred=1, bo='<', streams=None, n_table=None, extra_tags=()):
    """The bytes of a classic tiled TIFF of ``img`` ((H, W) or (H, W, spp), uint8 / uint16).  ``streams``: the tiles' bytes instead of
    the writer's own (damaged ones); ``n_table``: the tile tables are cut to so many entries; ``extra_tags``: (tag, type, values)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W, spp = img.shape
    bits = 8 * img.dtype.itemsize
    if streams is None:
        streams = tile_streams(img, th, tw, comp, pred, bo)
    body, offs = b'', []
    for s in streams:
        offs.append(8 + len(body))
        body += s + b'\0' * (len(s) & 1)
    cnts = [len(s) for s in streams]
    if n_table is not None:
        offs, cnts = offs[:n_table], cnts[:n_table]
    tags = [(256, 4, [W]), (257, 4, [H]), (258, 3, [bits] * spp), (259, 3, [comp]), (262, 3, [1 if spp == 1 else 2]), (277, 3, [spp]),
            (284, 3, [1]), (317, 3, [pred]), (322, 4, [tw]), (323, 4, [th]), (324, 4, offs), (325, 4, cnts), (339, 3, [1] * spp)]
    if spp == 4:
        tags.append((338, 3, [2]))
    tags = sorted(tags + list(extra_tags))
    ifd_off = 8 + len(body)
    extra_off = ifd_off + 2 + 12 * len(tags) + 4
    extra, entries = b'', b''
    for tag, typ, vals in tags:
        fmt = {3: 'H', 4: 'I'}[typ]
        data = struct.pack(bo + fmt * len(vals), *vals)
        if len(data) <= 4:
            field = data + b'\0' * (4 - len(data))
        else:
            field = struct.pack(bo + 'I', extra_off + len(extra))
            extra += data + b'\0' * (len(data) & 1)
        entries += struct.pack(bo + 'HHI', tag, typ, len(vals)) + field
    head = (b'II' if bo == '<' else b'MM') + struct.pack(bo + 'HI', 42, ifd_off)
    return head + body + struct.pack(bo + 'H', len(tags)) + entries + struct.pack(bo + 'I', 0) + extra


def case_name(kind, ext, comp, pred, bo):
    return '%s_%dx%d_t%dx%d_%s_p%d_%s' % (kind, ext[0], ext[1], ext[2], ext[3], comp, pred, 'le' if bo == '<' else 'be')


def all_cases():
    """(name, pixels (H, W, spp), file bytes) over every extent, with the sample, coding, predictor and byte-order variants spread over
    them so that each extent sees every variant of each axis and the whole stays a few hundred small files."""
    out = []
    k = 0
    for ext in EXTENTS:
        for kind in KINDS:
            for comp in COMPRESSIONS:
                pred = 1 + (k % 2)
                bo = '<' if (k // 2) % 2 == 0 else '>'
                k += 1
                for pr, b in ((pred, bo), (3 - pred, '>' if bo == '<' else '<')):
                    img = pixels(kind, ext[0], ext[1])
                    out.append((case_name(kind, ext, comp, pr, b), img, tiled_tiff(img, ext[2], ext[3], COMPRESSIONS[comp], pr, b)))
    return out


def fixture_cases():
    """The handful stored under tests/golden/tiff_tiles/: name -> (pixels, file bytes)."""
    picks = (('rgb8', EXTENTS[2], 'lzw', 2, '<'), ('gray16', EXTENTS[3], 'deflate', 2, '>'), ('rgba8', EXTENTS[1], 'raw', 1, '<'),
             ('rgb16', EXTENTS[6], 'lzw', 1, '>'), ('gray8', EXTENTS[4], 'deflate', 1, '<'))
    out = {}
    for kind, ext, comp, pred, bo in picks:
        img = pixels(kind, ext[0], ext[1])
        out[case_name(kind, ext, comp, pred, bo)] = (img, tiled_tiff(img, ext[2], ext[3], COMPRESSIONS[comp], pred, bo))
    return out


def squeeze(img):
    return img[..., 0] if img.shape[2] == 1 else img


# ---- files the parser must leave to the Python reader, and damaged files -------------------------------------------------------------
def refused_cases():
    """name -> file bytes of tiled files the device reader does not take even with the option on (ECSEG_E_UNSUPPORTED)."""
    img = pixels('rgb8', 33, 70)
    g = pixels('gray8', 33, 70)
    ok = tile_streams(img, 16, 16, 5, 1, '<')
    out = {
        'tile_width_24': tiled_tiff(img, 16, 24, 5),                                        # not a multiple of 16
        'tile_length_8': tiled_tiff(img, 8, 16, 5),
        'packbits_tiles': tiled_tiff(g, 16, 16, 32773, streams=[b'\x81\x00'] * 15),
        'short_tile_table': tiled_tiff(img, 16, 16, 5, streams=ok, n_table=len(ok) - 1),
        'strip_and_tile_tags': tiled_tiff(img, 16, 16, 5, extra_tags=[(273, 4, [8]), (279, 4, [10])]),
    }
    planar = bytearray(tiled_tiff(img, 16, 16, 1))
    at = planar.index(struct.pack('<HHIH', 284, 3, 1, 1))
    planar[at + 8] = 2
    out['planar_rgb'] = bytes(planar)
    big = bytearray(tiled_tiff(g, 16, 16, 1))
    big[2] = 43
    out['bigtiff_magic'] = bytes(big)
    f = bytearray(tiled_tiff(g, 16, 16, 1))
    at = f.index(struct.pack('<HHIH', 339, 3, 1, 1))
    f[at + 8] = 3
    out['float_samples'] = bytes(f)
    return out


def damaged_cases():
    """name -> (pixels or None, file bytes, which tile is hit): structurally tiled files whose verdict is the Python reader's."""
    img = pixels('rgb8', 33, 70, seed=3)
    out = {}
    lz = tile_streams(img, 16, 16, 5, 2, '<')
    bad = list(lz)
    bad[7] = bytes([0x80, 0x7f, 0xff, 0xff]) + bad[7][4:]        # ClearCode, then code 0x1ff...: an entry the table does not have
    out['corrupt_lzw_tile'] = (img, tiled_tiff(img, 16, 16, 5, 2, streams=bad), 7)
    zl = tile_streams(img, 16, 16, 8, 2, '<')
    bad = list(zl)
    bad[3] = bad[3][:-2] + bytes([bad[3][-2] ^ 0x55, bad[3][-1]])          # a wrong Adler-32
    out['corrupt_zlib_tile'] = (img, tiled_tiff(img, 16, 16, 8, 2, streams=bad), 3)
    bad = list(zl)
    bad[9] = bad[9][:len(bad[9]) // 2]                                   # a stream cut short
    out['short_zlib_tile'] = (img, tiled_tiff(img, 16, 16, 8, 2, streams=bad), 9)
    for name, comp, streams in (('lzw_offset_behind_file', 5, lz), ('zlib_offset_behind_file', 8, zl), ('raw_offset_behind_file', 1, None)):
        f = bytearray(tiled_tiff(img, 16, 16, comp, 2, streams=streams))
        offs_at = struct.unpack_from('<I', f, f.index(struct.pack('<HHI', 324, 4, 15)) + 8)[0]
        struct.pack_into('<I', f, offs_at + 4 * 5, len(f) + 1000)        # tile 5 starts behind the file
        out[name] = (img, bytes(f), 5)
    f = bytearray(tiled_tiff(img, 16, 16, 5, 2, streams=lz))
    cnts_at = struct.unpack_from('<I', f, f.index(struct.pack('<HHI', 325, 4, 15)) + 8)[0]
    struct.pack_into('<I', f, cnts_at + 4 * 14, 1 << 30)                 # the last tile's count leaves the file: clamped
    out['lzw_count_leaves_file'] = (img, bytes(f), 14)
    return out


def python_verdict(data, tmp_path, name='case'):
    """What image_io.read_tiff makes of the file: ('ok', array) or ('error', the exception)."""
    from ecseg_amd import image_io
    path = os.path.join(str(tmp_path), name + '.tif')
    with open(path, 'wb') as f:
        f.write(data)
    try:
        return 'ok', image_io.read_tiff(path, native=False)
    except (image_io.TiffError, zlib.error, IndexError) as e:    # a corrupt LZW stream; zlib's own error; a tile the table does not have
        return 'error', e
