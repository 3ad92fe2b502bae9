"""Deflate strips for the device TIFF reader's tests: a small bit writer that emits hand-built zlib streams - zlib itself never
writes most of them - and zlib's own output at the settings that give every kind of block.  Used by tests/test_tiff_inflate.py (the
strip routine on the host, under the sanitizers, and the host reader's verdicts) and tests/test_gpu_tiff_inflate.py (the device).

A case is (name, stream, want, cls, out): the strip's bytes, the bytes the strip holds, the class the host rule puts it in (the
names tools/asan/tiff_inflate_fuzz.cpp prints: 'ok: ...' or 'corrupt: ...') and, for an OK case, the bytes the stream gives (the
reader zero-fills up to ``want`` and cuts at it)."""
import zlib

import numpy as np

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
OK_EXACT = "ok: a complete stream of the strip's size"
OK_SHORT = 'ok: a complete stream shorter than the strip'
OK_FULL = 'ok: the strip is full before the stream ends'
OK_DRY = 'ok: out of input with the strip full'
TRUNCATED = 'corrupt: the stream ends before the strip is full'
CORRUPT_CLASSES = (
    'FDICT set', 'incorrect header check', 'unknown compression method', 'invalid window size', 'invalid block type',
    'invalid stored block lengths', 'too many length or distance symbols', 'invalid code lengths set', 'invalid bit length repeat',
    'invalid code -- missing end-of-block', 'invalid literal/lengths set', 'invalid distances set', 'invalid literal/length code',
    'invalid distance code', 'invalid distance too far back', 'incorrect data check')
ALL_CLASSES = (OK_EXACT, OK_SHORT, OK_FULL, OK_DRY, TRUNCATED) + tuple('corrupt: ' + c for c in CORRUPT_CLASSES)


class Bits:
    """Deflate's bit order: values from the least significant bit on, Huffman codes from their most significant bit on."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, length):
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def bytes(self):
        return bytes(self.align().out)


def canonical(lens):
    """Code lengths by symbol -> {symbol: (code, length)}, the canonical code (of an incomplete set too)."""
    code, out = 0, {}
    for length in range(1, 16):
        for sym, l in enumerate(lens):
            if l == length:
                out[sym] = (code, length)
                code += 1
        code <<= 1
    return out


def _length_symbol(n):
    """A match length 3..258 -> (symbol, extra bits, their value)."""
    if n == 258:
        return 285, 0, 0
    k = n - 3
    if k < 8:
        return 257 + k, 0, 0
    e = k.bit_length() - 3
    return 257 + 4 * (e + 1) + ((k >> e) & 3), e, k & ((1 << e) - 1)


def _distance_symbol(d):
    k = d - 1
    if k < 4:
        return k, 0, 0
    e = k.bit_length() - 2
    return 2 * (e + 1) + ((k >> e) & 1), e, k & ((1 << e) - 1)


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def stored(w, data, last=0, nlen=None):
    w.bits(last, 1).bits(0, 2).align()
    w.bits(len(data), 16).bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    return w.raw(data)


def symbols(w, items, lit, dist):
    """items: an int is a literal / end-of-block / raw symbol, (length, distance) a match, ('d', symbol) a raw distance symbol."""
    for it in items:
        if isinstance(it, int):
            w.code(*lit[it])
        elif it[0] == 'd':
            w.code(*dist[it[1]])
        else:
            s, e, v = _length_symbol(it[0])
            w.code(*lit[s]).bits(v, e)
            s, e, v = _distance_symbol(it[1])
            w.code(*dist[s]).bits(v, e)
    return w


def fixed(w, items, last=1):
    return symbols(w.bits(last, 1).bits(1, 2), items, FIXED_LIT, FIXED_DIST)


def run_tokens(lens):
    """Code lengths -> code-length symbols, greedy: (symbol, extra value) with zeros in 17 / 18 runs and repeats in 16 runs."""
    out, i = [], 0
    while i < len(lens):
        v, n = lens[i], 1
        while i + n < len(lens) and lens[i + n] == v:
            n += 1
        i += n
        if v == 0:
            while n >= 11:
                t = min(n, 138)
                out.append((18, t - 11))
                n -= t
            if n >= 3:
                out.append((17, n - 3))
                n = 0
            out += [(0, 0)] * n
        else:
            out.append((v, 0))
            n -= 1
            while n >= 3:
                t = min(n, 6)
                out.append((16, t - 3))
                n -= t
            out += [(v, 0)] * n
    return out


def dynamic_header(w, lit_lens, dist_lens, last=1, tokens=None, cl_lens=None, hlit=None, hdist=None, hclen=None):
    """The header of a dynamic block.  ``tokens``: the code-length symbols instead of the greedy ones; ``cl_lens``: the code-length
    code's lengths by symbol instead of a flat code over the symbols in use; hlit / hdist / hclen: the raw header fields."""
    tokens = run_tokens(list(lit_lens) + list(dist_lens)) if tokens is None else tokens
    if cl_lens is None:
        used = sorted({s for s, _ in tokens})
        width = max(1, (len(used) - 1).bit_length())
        cl_lens = [0] * 19
        for s in used:
            cl_lens[s] = width
        for s in range(19):                                      # pad the set to a complete one with symbols nobody writes
            if sum(1 for l in cl_lens if l) >= 1 << width:
                break
            if not cl_lens[s]:
                cl_lens[s] = width
    ncode = max([4] + [k + 1 for k, s in enumerate(ORDER) if cl_lens[s]])
    w.bits(last, 1).bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5).bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    w.bits(ncode - 4 if hclen is None else hclen, 4)
    for k in range(ncode if hclen is None else hclen + 4):
        w.bits(cl_lens[ORDER[k]], 3)
    cl = canonical(cl_lens)
    extra = {16: 2, 17: 3, 18: 7}
    for s, v in tokens:
        w.code(*cl[s]).bits(v, extra.get(s, 0))
    return w


def zwrap(body, data, head=b'\x78\x9c', check=None):
    return head + body + (zlib.adler32(data) if check is None else check).to_bytes(4, 'big')


def noise(seed, n, top=256):
    return np.random.default_rng(seed).integers(0, top, n, dtype=np.uint8).tobytes()


def _lens(pairs, n):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


def hand_cases():
    """[(name, stream, want, cls, out)]: what zlib never writes, and one stream at least of every class."""
    c = []
    add = lambda name, stream, want, cls, out=None: c.append((name, stream, want, cls, out))
    a4 = b'aaaa'
    # ---- well-formed rarities ----
    body = fixed(stored(Bits(), b''), [97, 98, 256]).bytes()
    add('stored_block_of_length_0', zwrap(body, b'ab'), 2, OK_EXACT, b'ab')
    body = fixed(stored(stored(stored(Bits(), b'xy'), b''), b'z'), [256]).bytes()
    add('stored_blocks_then_an_empty_fixed_block', zwrap(body, b'xyz'), 3, OK_EXACT, b'xyz')
    body = fixed(Bits(), [97, (258, 1), 256]).bytes()
    add('fixed_match_258_at_distance_1', zwrap(body, b'a' * 259), 259, OK_EXACT, b'a' * 259)
    add('fixed_match_258_into_a_shorter_strip', zwrap(body, b'a' * 259), 100, OK_FULL, b'a' * 100)
    add('fixed_match_258_into_a_longer_strip', zwrap(body, b'a' * 259), 300, OK_SHORT, b'a' * 259)
    body = fixed(Bits(), [97, 98, 99, (7, 3), (5, 2), 256]).bytes()
    add('overlapping_matches_at_distance_3_and_2', zwrap(body, b'abcabcabca' + b'cacac'), 15, OK_EXACT, b'abcabcabca' + b'cacac')
    far = noise(5, 32768)
    tail = far[:9]
    body = fixed(stored(Bits(), far), [(9, 32768), 256]).bytes()
    add('distance_32768_in_a_strip_above_32k', zwrap(body, far + tail), 32768 + 9, OK_EXACT, far + tail)
    body = fixed(stored(Bits(), far[:32767]), [(9, 32768), 256]).bytes()
    add('distance_one_byte_too_far', zwrap(body, far[:32767]), 32767 + 9, 'corrupt: invalid distance too far back')
    add('distance_2_behind_one_byte', zwrap(fixed(Bits(), [97, (3, 2), 256]).bytes(), a4), 4, 'corrupt: invalid distance too far back')
    add('too_far_back_but_the_strip_is_full', zwrap(fixed(Bits(), [97, (3, 2), 256]).bytes(), a4), 1, OK_FULL, b'a')
    # a dynamic block whose 16-run of length 2 crosses from the literal/length lengths (256, 257) into the four distance lengths
    lit = _lens([(97, 1), (256, 2), (257, 2)], 258)
    dist = [2, 2, 2, 2]
    tokens = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (2, 0), (16, 5 - 3)]
    w = dynamic_header(Bits(), lit, dist, tokens=tokens)
    body = symbols(w, [97, (3, 1), 256], canonical(lit), canonical(dist)).bytes()
    add('run_crossing_from_lengths_into_distances', zwrap(body, a4), 4, OK_EXACT, a4)
    tokens = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (2, 0), (2, 0), (18, 30 - 11)]      # a zero run over all 30 distance lengths
    w = dynamic_header(Bits(), lit, [0] * 30, tokens=tokens)
    body = symbols(w, [97, 97, 256], canonical(lit), {}).bytes()
    add('zero_code_distance_alphabet_literals_only', zwrap(body, b'aa'), 2, OK_EXACT, b'aa')
    w = dynamic_header(Bits(), lit, [0])
    add('zero_code_distance_alphabet_with_a_match', zwrap(symbols(w, [97, 257], canonical(lit), {}).bits(0, 8).bytes(), a4), 4, 'corrupt: invalid distance code')
    w = dynamic_header(Bits(), lit, [1])
    add('one_code_distance_alphabet', zwrap(symbols(w, [97, (3, 1), 256], canonical(lit), canonical([1])).bytes(), a4), 4, OK_EXACT, a4)
    w = dynamic_header(Bits(), lit, [1])
    add('one_code_distance_alphabet_the_other_bit', zwrap(symbols(w, [97, 257], canonical(lit), {}).bits(1, 1).bits(0, 8).bytes(), a4), 4,
        'corrupt: invalid distance code')
    one = _lens([(256, 1)], 257)
    add('one_code_literal_alphabet_only_end_of_block', zwrap(symbols(dynamic_header(Bits(), one, [0]), [256], canonical(one), {}).bytes(), b''), 3, OK_SHORT, b'')
    add('one_code_literal_alphabet_the_other_bit', zwrap(dynamic_header(Bits(), one, [0]).bits(1, 1).bits(0, 8).bytes(), b''), 3, 'corrupt: invalid literal/length code')
    # ---- the strip full, and the stream going on ----
    body = fixed(stored(fixed(Bits(), [97, 98, 256], last=0), b'', last=0), [256]).bytes()
    add('empty_blocks_behind_a_full_strip', zwrap(body, b'ab'), 2, OK_EXACT, b'ab')
    add('wrong_check_behind_a_full_strip', zwrap(body, b'ab', check=1), 2, 'corrupt: incorrect data check')
    add('trailer_cut_behind_a_full_strip', zwrap(body, b'ab')[:-2], 2, OK_DRY, b'ab')
    add('block_type_3_behind_a_full_strip', b'\x78\x9c' + fixed(Bits(), [97, 98, 256], last=0).bits(0, 1).bits(3, 2).bytes(), 2, 'corrupt: invalid block type')
    add('more_literals_behind_a_full_strip', zwrap(fixed(Bits(), [97, 98, 99, 100, 256]).bytes(), b'abcd'), 2, OK_FULL, b'ab')
    add('a_bad_distance_code_behind_a_full_strip', b'\x78\x9c' + fixed(Bits(), [97, 257, ('d', 30)]).bits(0, 16).bytes(), 1, 'corrupt: invalid distance code')
    # ---- every corrupt class ----
    good = zwrap(fixed(Bits(), [97, 98, 256]).bytes(), b'ab')
    add('header_check', b'\x78\x9d' + good[2:], 2, 'corrupt: incorrect header check')
    add('compression_method_7', b'\x77\x09' + good[2:], 2, 'corrupt: unknown compression method')
    add('window_of_64k', b'\x88\x1c' + good[2:], 2, 'corrupt: invalid window size')
    add('fdict', b'\x78\xbb' + b'\0\0\0\1' + good[2:], 2, 'corrupt: FDICT set')
    add('block_type_3', b'\x78\x9c' + Bits().bits(1, 1).bits(3, 2).bits(0, 13).bytes(), 2, 'corrupt: invalid block type')
    add('stored_len_nlen', b'\x78\x9c' + stored(Bits(), b'ab', last=1, nlen=0x1234).bytes() + b'\0\0\0\0', 2, 'corrupt: invalid stored block lengths')
    add('hlit_287', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], hlit=30).bits(0, 32).bytes(), 4, 'corrupt: too many length or distance symbols')
    add('hdist_31', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], hdist=30).bits(0, 32).bytes(), 4, 'corrupt: too many length or distance symbols')
    over = [0] * 19
    over[0] = over[1] = over[2] = 1
    add('code_length_code_over_subscribed', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], tokens=[], cl_lens=over).bits(0, 32).bytes(), 4, 'corrupt: invalid code lengths set')
    under = [0] * 19
    under[0] = 1
    add('code_length_code_incomplete', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], tokens=[], cl_lens=under).bits(0, 32).bytes(), 4, 'corrupt: invalid code lengths set')
    flat = [0] * 19
    flat[16] = flat[18] = flat[1] = flat[2] = 2
    add('repeat_with_nothing_before_it', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], tokens=[(16, 0)], cl_lens=flat).bits(0, 32).bytes(), 4, 'corrupt: invalid bit length repeat')
    add('run_past_the_last_length', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], tokens=[(18, 127), (18, 127)], cl_lens=flat).bits(0, 32).bytes(), 4,
        'corrupt: invalid bit length repeat')
    none = _lens([(97, 1), (98, 1)], 257)
    add('no_end_of_block_code', b'\x78\x9c' + dynamic_header(Bits(), none, [1]).bits(0, 32).bytes(), 4, 'corrupt: invalid code -- missing end-of-block')
    add('empty_code_length_code', b'\x78\x9c' + dynamic_header(Bits(), lit, [1], tokens=[], cl_lens=[0] * 19).bits(0, 320).bytes(), 4,
        'corrupt: invalid code -- missing end-of-block')
    big = _lens([(97, 1), (98, 1), (256, 1)], 257)
    add('literal_lengths_over_subscribed', b'\x78\x9c' + dynamic_header(Bits(), big, [1]).bits(0, 32).bytes(), 4, 'corrupt: invalid literal/lengths set')
    thin = _lens([(97, 2), (256, 2)], 257)
    add('literal_lengths_incomplete', b'\x78\x9c' + dynamic_header(Bits(), thin, [1]).bits(0, 32).bytes(), 4, 'corrupt: invalid literal/lengths set')
    add('distance_lengths_over_subscribed', b'\x78\x9c' + dynamic_header(Bits(), lit, [1, 1, 1]).bits(0, 32).bytes(), 4, 'corrupt: invalid distances set')
    add('distance_lengths_incomplete', b'\x78\x9c' + dynamic_header(Bits(), lit, [2, 2]).bits(0, 32).bytes(), 4, 'corrupt: invalid distances set')
    add('symbol_286', b'\x78\x9c' + fixed(Bits(), [97, 286]).bits(0, 16).bytes(), 4, 'corrupt: invalid literal/length code')
    add('symbol_287', b'\x78\x9c' + fixed(Bits(), [97, 287]).bits(0, 16).bytes(), 4, 'corrupt: invalid literal/length code')
    add('distance_code_30', b'\x78\x9c' + fixed(Bits(), [97, 257, ('d', 30)]).bits(0, 16).bytes(), 4, 'corrupt: invalid distance code')
    add('distance_code_31', b'\x78\x9c' + fixed(Bits(), [97, 257, ('d', 31)]).bits(0, 16).bytes(), 4, 'corrupt: invalid distance code')
    add('wrong_adler', zwrap(fixed(Bits(), [97, 98, 256]).bytes(), b'ab', check=0x12345678), 2, 'corrupt: incorrect data check')
    add('wrong_adler_in_a_longer_strip', zwrap(fixed(Bits(), [97, 98, 256]).bytes(), b'ab', check=0x12345678), 9, 'corrupt: incorrect data check')
    # ---- the class the stated rule decides: the stream ends before the strip is full and before its own end ----
    add('cut_inside_the_symbols', good[:3], 2, TRUNCATED)
    add('cut_inside_the_header', good[:1], 2, TRUNCATED)
    add('cut_inside_the_trailer_of_a_short_stream', good[:-1], 5, TRUNCATED)
    add('cut_inside_a_stored_block', b'\x78\x9c' + stored(Bits(), b'abcdef', last=1).bytes()[:-2], 6, TRUNCATED)
    add('empty_strip', b'', 2, TRUNCATED)
    return c


def zlib_streams():
    """[(name, stream, want, cls, out)]: zlib's own output - level 0 (stored blocks), Z_FIXED, level 9 on noise (dynamic blocks that
    are nearly literal), several blocks per strip behind full flushes, long runs (matches of 258 at distance 1), and a text-like buffer
    whose distances go far - into destinations of the exact, a larger and a smaller size."""
    def deflated(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, pieces=1):
        z = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        out = b''
        for k in range(pieces):
            out += z.compress(data[len(data) * k // pieces:len(data) * (k + 1) // pieces])
            if k + 1 < pieces:
                out += z.flush(zlib.Z_FULL_FLUSH)
        return out + z.flush()
    text = (noise(7, 300, 4) * 40 + noise(8, 2000, 16)) * 3
    kinds = (('level_0', noise(1, 70000), 0, zlib.Z_DEFAULT_STRATEGY, 1), ('fixed', noise(2, 5000, 6), 6, zlib.Z_FIXED, 1),
             ('level_9_on_noise', noise(3, 40000), 9, zlib.Z_DEFAULT_STRATEGY, 1), ('five_blocks', text, 6, zlib.Z_DEFAULT_STRATEGY, 5),
             ('zeros', bytes(100000), 9, zlib.Z_DEFAULT_STRATEGY, 1), ('text', text, 9, zlib.Z_DEFAULT_STRATEGY, 1),
             ('huffman_only', noise(4, 9000, 20), 6, zlib.Z_HUFFMAN_ONLY, 2), ('one_byte', b'q', 6, zlib.Z_DEFAULT_STRATEGY, 1))
    c = []
    for name, data, level, strategy, pieces in kinds:
        z = deflated(data, level, strategy, pieces)
        c.append((name, z, len(data), OK_EXACT, data))
        c.append((name + '_short', z, len(data) + 77, OK_SHORT, data))
        if len(data) > 1:
            c.append((name + '_long', z, len(data) * 2 // 3, OK_FULL, data[:len(data) * 2 // 3]))
            c.append((name + '_cut', z[:len(z) // 2], len(data), TRUNCATED, None))
    return c


def mutations(n=300, seed=1729):
    """[(name, stream, want)]: seeded bit flips (half of them in the first 40 bytes, where the headers and tables lie), truncations and
    spliced headers of three of zlib's streams; their class is whatever the host rule says."""
    rng = np.random.default_rng(seed)
    base = [(s, w) for name, s, w, _, _ in zlib_streams() if name in ('fixed', 'five_blocks', 'level_9_on_noise', 'huffman_only')]
    out = []
    for k in range(n):
        s, want = base[k % len(base)]
        b = bytearray(s)
        kind = k % 3
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, min(len(b), 40) if k % 2 else len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            other = base[(k + 1) % len(base)][0]
            head = int(rng.integers(2, min(len(other), len(b), 200)))
            b[:head] = other[:head]
        out.append(('mutation_%d' % k, bytes(b), want if k % 5 else max(1, want // 2)))
    return out
