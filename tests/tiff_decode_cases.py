"""Inputs of the device TIFF reader's tests (csrc/tiff_decode_kernels.hip): LZW streams as code lists, packed by the decoder's own
width schedule so that any list is readable; whole TIFF files around given strips; the tolerated streams and the seeded corrupt
corpus that tests/test_tiff_decode.py runs through the sanitizer program and tests/test_gpu_tiff_decode.py through the device.
The expected value is never built here: it is what the host decoder makes of the same bytes."""
import struct

import numpy as np

CLEAR, EOI = 256, 257


def lzw_codes(data, restart=True):
    """bytes -> the code list of greedy TIFF LZW, ClearCode first, EOI last.  ``restart``: a ClearCode and a fresh table when the next
    entry would be 4094 (libtiff's rule, tests/lzw_ref.py); without it the table fills to 4096 entries and stops growing."""
    codes, table, nxt = [CLEAR], {}, 258
    if len(data):
        cur = data[0]
        for c in data[1:]:
            key = (cur << 8) | c
            hit = table.get(key)
            if hit is not None:
                cur = hit
                continue
            codes.append(cur)
            if nxt < 4096:
                table[key] = nxt
                nxt += 1
            if restart and nxt == 4094:
                codes.append(CLEAR)
                table, nxt = {}, 258
            cur = c
        codes.append(cur)
    codes.append(EOI)
    return codes


def pack(codes):
    """A code list -> bytes, MSB first, every code at the width the decoder reads it with (early change)."""
    acc = nbits = 0
    out = bytearray()
    width, nxt, old = 9, 258, False
    for code in codes:
        acc = (acc << width) | code
        nbits += width
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xff)
            nbits -= 8
        acc &= (1 << nbits) - 1
        if code == CLEAR:
            width, nxt, old = 9, 258, False
        elif code != EOI:
            if not old:
                old = True
                continue
            if nxt < 4096:
                nxt += 1
            if nxt >= (1 << width) - 1 and width < 12:
                width += 1
    if nbits:
        out.append((acc << (8 - nbits)) & 0xff)
    return bytes(out)


def tiff_file(strips, H, W, rps, spp=1, bits=8, compression=5, predictor=1, counts=None, offsets=None, big_endian=False):
    """A classic TIFF of 1 or 3 samples per pixel around ``strips`` (their bytes as given).  ``counts`` / ``offsets``: what the tables say instead of the truth
    (shorter lists make shorter tables)."""
    bo = '>' if big_endian else '<'
    body, offs, pos = b'', [], 8
    for s in strips:
        offs.append(pos)
        body += s + (b'\0' if len(s) & 1 else b'')
        pos += len(s) + (len(s) & 1)
    offs = list(offsets) if offsets is not None else offs
    cnts = list(counts) if counts is not None else [len(s) for s in strips][:len(offs)]
    offs = offs[:len(cnts)]
    n = len(offs)
    extra = b''
    so, sc, bps = offs[0], cnts[0], bits
    if n > 1:
        so = pos + len(extra)
        extra += struct.pack(bo + '%dI' % n, *offs)
        sc = pos + len(extra)
        extra += struct.pack(bo + '%dI' % n, *cnts)
    if spp > 2:
        bps = pos + len(extra)
        extra += struct.pack(bo + '%dH' % spp, *([bits] * spp))
    ifd_off = pos + len(extra)
    pad = b'\0' if ifd_off & 1 else b''
    ifd_off += len(pad)

    def entry(tag, typ, count, value):
        if typ == 3 and count == 1:                              # a SHORT lies in the first two bytes of the value field
            return struct.pack(bo + 'HHIHH', tag, typ, count, value, 0)
        return struct.pack(bo + 'HHII', tag, typ, count, value)
    entries = [(256, 4, 1, W), (257, 4, 1, H), (258, 3, spp, bps), (259, 3, 1, compression), (262, 3, 1, 1 if spp < 3 else 2),
               (273, 4, n, so), (277, 3, 1, spp), (278, 4, 1, rps), (279, 4, n, sc), (284, 3, 1, 1), (317, 3, 1, predictor), (339, 3, 1, 1)]
    ifd = struct.pack(bo + 'H', len(entries)) + b''.join(entry(*e) for e in entries) + struct.pack(bo + 'I', 0)
    return (b'MM' if big_endian else b'II') + struct.pack(bo + 'HI', 42, ifd_off) + body + extra + pad + ifd


def _noise(seed, n, top=256):
    return np.random.default_rng(seed).integers(0, top, n, dtype=np.uint8).tobytes()


def tolerated_files():
    """[(name, file bytes)]: the streams the host decoder accepts beside a well-formed one, each as the strips of a gray file."""
    small = _noise(31, 40 * 50, 7)                               # 40 x 50, strings of several bytes
    codes = lzw_codes(small)
    long = _noise(32, 2 * 12000)                                 # noise: the table restarts inside the strip
    restarted = lzw_codes(long)
    at = restarted.index(CLEAR, 1)
    full = lzw_codes(long, restart=False)
    assert CLEAR not in full[1:] and len(full) > 4096 + 300
    three = [pack(lzw_codes(small[r * 50:(r + 10) * 50])) for r in (0, 10, 20, 30)]      # strips of ten rows
    one = pack(codes)
    return [
        ('well_formed', tiff_file([one], 40, 50, 40)),
        ('no_leading_clearcode', tiff_file([pack(codes[1:])], 40, 50, 40)),
        ('no_eoi', tiff_file([pack(codes[:-1])], 40, 50, 40)),
        ('byte_count_cut_short', tiff_file([one], 40, 50, 40, counts=[len(one) * 2 // 3])),
        ('strip_holds_more_than_want', tiff_file([one], 31, 50, 31)),
        ('strip_ends_inside_a_string', tiff_file([one], 39, 51, 39)),
        ('two_clearcodes_in_a_row', tiff_file([pack([CLEAR] + codes)], 40, 50, 40)),
        ('two_clearcodes_at_a_restart', tiff_file([pack(restarted[:at] + [CLEAR] + restarted[at:])], 2, 12000, 2)),
        ('table_full_without_clearcode', tiff_file([pack(full)], 2, 12000, 2)),
        ('table_shorter_than_the_image', tiff_file(three[:3], 40, 50, 10, counts=[len(s) for s in three[:2]])),
        ('empty_strip', tiff_file([b''], 4, 4, 4)),
    ]


def offset_behind_the_file():
    one = pack(lzw_codes(_noise(33, 200)))
    return tiff_file([one, one], 20, 20, 10, offsets=[8, 1 << 20])


def corrupt_corpus(n=200, seed=4711):
    """[(name, file bytes)]: seeded truncations and single-bit flips of the strip data of three small files - gray 31 x 257 (one
    strip), RGB 5 x 7, 16-bit gray with the predictor (two strips) -, ``n`` in all.  The tables keep the original counts."""
    rng = np.random.default_rng(seed)
    gray = rng.integers(0, 256, 31 * 257, dtype=np.uint8).tobytes()
    rgb = rng.integers(0, 8, 5 * 7 * 3, dtype=np.uint8).tobytes()
    g16 = np.diff(rng.integers(0, 3000, (12, 40), dtype=np.uint16), axis=1, prepend=np.uint16(0)).astype('<u2')
    bases = [
        ('gray_31x257', [pack(lzw_codes(gray))], dict(H=31, W=257, rps=31)),
        ('rgb_5x7', [pack(lzw_codes(rgb))], dict(H=5, W=7, rps=5, spp=3, predictor=2)),
        ('gray16_predictor', [pack(lzw_codes(g16[:6].tobytes())), pack(lzw_codes(g16[6:].tobytes()))], dict(H=12, W=40, rps=6, bits=16, predictor=2)),
    ]
    out = []
    for i in range(n):
        name, strips, kw = bases[i % 3]
        strips = [bytearray(s) for s in strips]
        k = int(rng.integers(0, len(strips)))
        counts = [len(s) for s in strips]
        if i % 2:
            at = int(rng.integers(0, len(strips[k]) * 8))
            strips[k][at >> 3] ^= 0x80 >> (at & 7)
            what = 'flip_%d' % at
        else:
            cut = int(rng.integers(0, len(strips[k])))
            counts[k] = cut
            what = 'cut_%d' % cut
        out.append(('%s_%03d_%s' % (name, i, what), tiff_file([bytes(s) for s in strips], counts=counts, **kw)))
    return out


def strips_of(data):
    """A file of ``tiff_file`` -> [(stream bytes as the reader clamps them, want)] per strip of the image: what the decoder gets."""
    bo = '<' if data[:2] == b'II' else '>'
    ifd = struct.unpack_from(bo + 'I', data, 4)[0]
    tags = {}
    for i in range(struct.unpack_from(bo + 'H', data, ifd)[0]):
        tag, typ, count = struct.unpack_from(bo + 'HHI', data, ifd + 2 + 12 * i)
        size = {3: 2, 4: 4}[typ]
        at = ifd + 2 + 12 * i + 8
        if size * count > 4:
            at = struct.unpack_from(bo + 'I', data, at)[0]
        tags[tag] = struct.unpack_from(bo + '%d%s' % (count, 'H' if typ == 3 else 'I'), data, at)
    H, W, spp, rps = tags[257][0], tags[256][0], tags[277][0], tags[278][0]
    line = W * spp * tags[258][0] // 8
    out = []
    for k, (o, c) in enumerate(zip(tags[273], tags[279])):
        rows = min(rps, H - k * rps)
        if rows <= 0 or o > len(data):
            break
        out.append((data[o:o + min(c, len(data) - o)], rows * line))
    return out


def file_of(img, rps, compression=5, predictor=1, big_endian=False):
    """the file of (H, W[, C]) uint8 / uint16 samples under a plan, strips by ``lzw_codes`` / ``pack``, the file by ``tiff_file``"""
    H, W = img.shape[:2]
    a = img.reshape(H, W, -1)
    if predictor == 2:
        d = a.copy()
        d[:, 1:] = a[:, 1:] - a[:, :-1]
        a = d
    if a.dtype == np.uint16:
        a = a.astype('>u2' if big_endian else '<u2')
    rows = a.reshape(H, -1)
    strips = [rows[r:r + rps].tobytes() for r in range(0, H, rps)]
    if compression == 5:
        strips = [pack(lzw_codes(s)) for s in strips]
    return tiff_file(strips, H, W, rps, spp=a.shape[2], bits=8 * img.dtype.itemsize, compression=compression, predictor=predictor, big_endian=big_endian)
