"""A plain Python restatement of the host's TIFF LZW encoder (ecseg_lzw_encode, csrc/host_codec.cpp) and of the file its writers
build around the strips (tiff_write_u8, csrc/host_io.cpp).  The dictionary is a Python dict: greedy LZW with fixed rules has one
output whatever finds the matches.  Besides the bytes, ``encode`` reports what a case list has to cover: how often the table was
restarted, the code width at EOI, whether ``last()`` stepped the width, and whether the length is odd."""
import struct
from collections import namedtuple

import numpy as np

Encoded = namedtuple('Encoded', 'data restarts eoi_width last_stepped odd restart_on_last_byte')
CLEAR, EOI = 256, 257


def encode(data, states=None):
    """bytes -> Encoded.  ``states``: a list that receives, after every byte but the first, (next, width, restarted at this byte) -
    the encoder's state if the strip ended there, before ``last()``."""
    out = bytearray()
    acc = nbits = 0
    width, nxt = 9, 258
    table = {}
    restarts = 0
    restarted = False

    def put(code):
        nonlocal acc, nbits
        acc = ((acc << width) | code) & 0xffffffffffffffff
        nbits += width
        if nbits >= 32:
            out.extend(struct.pack('>I', (acc >> (nbits - 32)) & 0xffffffff))
            nbits -= 32

    put(CLEAR)
    last_stepped = False
    if len(data):
        cur = data[0]
        for c in data[1:]:
            key = (cur << 8) | c
            hit = table.get(key)
            restarted = False
            if hit is not None:
                cur = hit
            else:
                put(cur)
                table[key] = nxt
                nxt += 1
                if nxt == 4094:                                  # table full: restart (libtiff's CODE_MAX - 1 rule)
                    put(CLEAR)
                    table = {}
                    nxt, width = 258, 9
                    restarts += 1
                    restarted = True
                elif nxt > (1 << width) - 1 and width < 12:
                    width += 1
                cur = c
            if states is not None:
                states.append((nxt, width, restarted))
        put(cur)                                                 # last(): the decoder adds one more entry after this code
        nxt += 1
        if nxt > (1 << width) - 1 and width < 12:
            width += 1
            last_stepped = True
    eoi_width = width
    put(EOI)
    while nbits > 0:                                             # the last 1..31 bits, zero-padded to a byte
        take = min(nbits, 8)
        out.append(((acc >> (nbits - 8)) if nbits >= 8 else (acc << (8 - nbits))) & 0xff)
        nbits -= take
    return Encoded(bytes(out), restarts, eoi_width, last_stepped, len(out) % 2 == 1, restarted)


def boundary_lengths(data):
    """One pass over ``data`` -> {what: n}: the shortest strip ``data[:n]`` at which ``last()`` steps the width 9 -> 10, 10 -> 11 and
    11 -> 12, and at which the table restart falls on the final byte (n = k + 1 for the byte k that creates entry 4093)."""
    states = []
    encode(data, states)
    found = {}
    for i, (nxt, width, restarted) in enumerate(states):
        n = i + 2                                                # states[i] is the state behind byte i + 1
        for w in (9, 10, 11):
            if width == w and nxt + 1 > (1 << w) - 1 and restarted is False:
                found.setdefault('last_%d_%d' % (w, w + 1), n)
        if restarted:
            found.setdefault('restart_last', n)
    return found


def rows_per_strip(H, line):
    return max(1, min(H, 8192 // line))


def strips(img, invert=False):
    """(H, W) or (H, W, 3) uint8 -> the predicted bytes of every strip: 255 - img under ``invert``, then per row a byte minus the
    byte spp to its left, the first spp bytes as they are."""
    a = np.ascontiguousarray(img, np.uint8)
    spp = 1 if a.ndim == 2 else a.shape[2]
    a = a.reshape(a.shape[0], -1)
    if invert:
        a = ~a
    d = a.copy()
    d[:, spp:] = a[:, spp:] - a[:, :-spp]
    rps = rows_per_strip(a.shape[0], a.shape[1])
    return [d[r:r + rps].tobytes() for r in range(0, a.shape[0], rps)]


def tiff_file(img, invert=False, encoded=None):
    """The whole file ecseg_tiff_write_gray8 / _rgb8 write: 8-byte header, the strips (a 0 behind an odd one), the offset and count
    tables (more than one strip), BitsPerSample (RGB), a pad to an even offset, the 12-entry IFD.  ``encoded``: the strips'
    ``Encoded`` if the caller has them."""
    a = np.ascontiguousarray(img, np.uint8)
    H, W = a.shape[:2]
    spp = 1 if a.ndim == 2 else a.shape[2]
    enc = [e.data for e in encoded] if encoded is not None else [encode(s).data for s in strips(a, invert)]
    n = len(enc)
    body, offs, pos = b'', [], 8
    for s in enc:
        offs.append(pos)
        body += s + (b'\0' if len(s) & 1 else b'')
        pos += len(s) + (len(s) & 1)
    extra = b''
    so, sc, bps = offs[0], len(enc[0]), 8
    if n > 1:
        so = pos + len(extra)
        extra += struct.pack('<%dI' % n, *offs)
        sc = pos + len(extra)
        extra += struct.pack('<%dI' % n, *[len(s) for s in enc])
    if spp > 2:
        bps = pos + len(extra)
        extra += struct.pack('<%dH' % spp, *([8] * spp))
    ifd_off = pos + len(extra)
    pad = b'\0' if ifd_off & 1 else b''
    ifd_off += len(pad)
    entries = [(256, 4, 1, W), (257, 4, 1, H), (258, 3, spp, bps), (259, 3, 1, 5), (262, 3, 1, 1 if spp == 1 else 2), (273, 4, n, so),
               (277, 3, 1, spp), (278, 4, 1, rows_per_strip(H, W * spp)), (279, 4, n, sc), (284, 3, 1, 1), (317, 3, 1, 2), (339, 3, 1, 1)]
    ifd = struct.pack('<H', len(entries)) + b''.join(struct.pack('<HHII', *e) for e in entries) + struct.pack('<I', 0)
    return b'II' + struct.pack('<HI', 42, ifd_off) + body + extra + pad + ifd
