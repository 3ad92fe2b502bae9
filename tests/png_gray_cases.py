"""The case list of the gray-channel PNG coder, shared by the CPU tests (tests/test_png_gray.py: the host writer, the yardstick) and
the GPU tests (tests/test_gpu_png_gray.py: ecseg_png_channel_encode).  A case is ``(name, pixels (n, H, W, C) uint8, channel, invert)``.

Cases are built from the FILTERED stream they are to have: ``n = H (W + 1)`` bytes, byte 0 of every scan line the filter byte 1, the
others the SUB differences of the channel's (optionally inverted) samples.  ``pixels_of_stream`` turns such a stream into pixels, so a
run that crosses a scan line (a line whose filtered tail is 1 and a next line that starts with sample 1) is written down as what it
is: ones around a multiple of ``W + 1``.  The device walks the flat stream 64 bytes per wave step and 1024 bytes per wave."""
import numpy as np

EXTENTS = [(1, 1), (1, 2), (3, 62), (3, 63), (3, 64), (5, 127), (4, 128), (2, 300), (33, 200), (70, 255)]
# ramp rows give an all-ones stream, one run of n bytes: n - 1 hits each branch of the match split (258, 259, 260, 261, 516, 517)
RAMP_EXTENTS = [(7, 36), (4, 64), (9, 28), (2, 130), (11, 46), (7, 73)]


def stream_of(channel, invert):
    """(H, W) uint8 samples -> the (H, W + 1) filtered scan lines: filter byte 1, then sample minus left neighbour (0 in front)"""
    v = np.asarray(channel, np.uint8) ^ np.uint8(255 if invert else 0)
    f = np.empty((v.shape[0], v.shape[1] + 1), np.uint8)
    f[:, 0] = 1
    f[:, 1] = v[:, 0]
    f[:, 2:] = v[:, 1:] - v[:, :-1]
    return f


def pixels_of_stream(flat, H, W, C, channel, invert, rng):
    """a flat stream (its filter bytes are overwritten with 1) -> (H, W, C) pixels whose channel has it; the other channels are noise"""
    f = np.array(flat, np.uint8).reshape(H, W + 1)
    v = np.cumsum(f[:, 1:].astype(np.uint64), axis=1).astype(np.uint8) ^ np.uint8(255 if invert else 0)
    px = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    px[..., channel] = v
    assert np.array_equal(stream_of(px[..., channel], invert)[:, 1:], f[:, 1:])
    return px


def runs_of(flat):
    """the maximal runs of a flat stream -> (starts, lengths)"""
    flat = np.asarray(flat).ravel()
    starts = np.flatnonzero(np.concatenate([[True], flat[1:] != flat[:-1]]))
    return starts, np.diff(np.concatenate([starts, [flat.size]]))


def split_branch(r):
    """which branch of the match split a run's r = R - 1 matched bytes take (the token rule of csrc/png_gray_tokens.h)"""
    if r < 3:
        return 'literals'
    if r <= 258:
        return 'one'
    t = r % 258
    return 'whole' if t == 0 else 'tail' if t >= 3 else 'short_tail_%d' % t


def tokens_of(flat):
    """the token rule restated on maximal runs: literal b as b, a distance-1 match of L bytes as -L"""
    flat = np.asarray(flat).ravel()
    out = []
    for s, R in zip(*runs_of(flat)):
        b = int(flat[s])
        if R < 4:
            out += [b] * int(R)
            continue
        r = int(R) - 1
        k, t = divmod(r, 258)
        out.append(b)
        if k == 0:
            out.append(-r)
        elif t == 0:
            out += [-258] * k
        elif t >= 3:
            out += [-258] * k + [-t]
        else:
            out += [-258] * (k - 1) + [-(255 + t), -3]
    return out


def _ramp(H, W):
    return np.ones(H * (W + 1), np.uint8)


def _noise_without_runs(H, W, rng):
    """uniform noise in which no byte repeats (the filter bytes then make runs of three at the most): no match is sent"""
    n = H * (W + 1)
    return np.cumsum(rng.integers(1, 256, n)).astype(np.uint8)


def fish_raster(H, W, rng):
    """clip(N(20, 8)) noise plus bright dots: an (H, W) uint8 channel (shared with tests/test_gpu_scratch.py)"""
    v = np.clip(rng.normal(20, 8, (H, W)), 0, 255).astype(np.uint8)
    for _ in range(max(1, H * W // 400)):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        v[y:y + 2, x:x + 2] = 230
    return v


def _fish(H, W, rng):
    """``fish_raster`` as the stream of its samples"""
    return stream_of(fish_raster(H, W, rng), False).ravel()


def _speckle(H, W, rng):
    """geometric runs over a small alphabet in which 1 is common, so runs cross scan lines"""
    n = H * (W + 1)
    lens = rng.geometric(0.2, n)
    vals = rng.integers(0, 3, n)
    return np.repeat(vals, lens)[:n].astype(np.uint8)


# Placed runs: one run of R equal bytes in a stream without other runs (2, 3, 2, 3, ... with the filter bytes 1 alone between them), at
# each of three placements against each of three borders.  The borders are a 64-byte step border, a 1024-byte span border and a
# scan-line end (the position of a filter byte); the placements are: the run starts on the border, ends on it (its last byte is the
# byte in front of it), straddles it (R // 2 bytes in front).  A run that covers a filter byte is a run of ones - that is what a run
# across a scan line is: a line whose filtered tail is 1 and a next line whose first sample is 1 - any other is a run of fives.
PLACED_EXTENT = (4, 1299)                                     # scan lines of 1300 bytes, 5200 in all: six spans
PLACED_LENGTHS = (1, 2, 3, 4, 5, 259, 260, 261, 262)
PLACED_BORDERS = {'block': 64 * 9, 'span': 1024, 'line': 2 * (PLACED_EXTENT[1] + 1)}
PLACEMENTS = ('start', 'end', 'straddle')


def placed_run(R, border, placement):
    """-> (first position, byte) of the run; None for a placement the length cannot have (one byte straddles nothing)"""
    if placement == 'straddle' and R < 2:
        return None
    b = PLACED_BORDERS[border]
    at = b if placement == 'start' else b - R if placement == 'end' else b - R // 2
    line = PLACED_EXTENT[1] + 1
    covers_filter_byte = (at + R - 1) // line != (at - 1) // line
    return at, 1 if covers_filter_byte else 5


def _placed_stream(R, border, placement):
    H, W = PLACED_EXTENT
    n = H * (W + 1)
    f = (2 + (np.arange(n) & 1)).astype(np.uint8)
    f[::W + 1] = 1
    at, byte = placed_run(R, border, placement)
    f[at:at + R] = byte
    starts, lens = runs_of(f)
    k = int(np.searchsorted(starts, at))
    assert starts[k] == at and lens[k] == R and (np.delete(lens, k) == 1).all()      # the run as placed, and no other
    return f


def _fibonacci(H, W):
    """literal counts that follow the Fibonacci numbers, no byte twice in a row (so no match is sent): the Huffman tree is a chain, and
    the code reaches huffman_lengths' limit of 15 bits"""
    n = H * (W + 1)
    fib = [1, 2]
    while sum(fib) + fib[-1] + fib[-2] <= n:
        fib.append(fib[-1] + fib[-2])
    counts = dict(zip(range(2, 2 + len(fib)), fib))           # byte -> count; byte 1, the filter byte's, takes over the first count above H
    k = min(b for b, c in counts.items() if c > H)
    counts[1] = counts.pop(k) - H
    order = sorted(counts, key=lambda b: -counts[b])
    seq = np.concatenate([np.full(counts[b], b) for b in order])
    seq = np.concatenate([seq, np.full(n - H - seq.size, order[0])])
    out = np.empty(n - H, np.int64)
    half = (n - H + 1) // 2
    out[0::2], out[1::2] = seq[:half], seq[half:]             # the commonest byte on even places, the others between: no neighbours are equal
    f = np.ones((H, W + 1), np.uint8)
    f[:, 1:] = out.reshape(H, W)
    return f.ravel()


def build_cases():
    rng = np.random.default_rng(20260901)
    cases = []
    k = 0

    def add(name, H, W, make, n_img=1):
        nonlocal k
        C = (2, 3, 4, 3)[k % 4]
        channel, invert = (k // 2) % 2, k % 2
        k += 1
        px = np.stack([pixels_of_stream(make(), H, W, C, channel, invert, rng) for _ in range(n_img)])
        cases.append(('%s_%dx%d_c%d_ch%d_inv%d_n%d' % (name, H, W, C, channel, invert, n_img), px, channel, invert))

    for H, W in EXTENTS:
        add('ramp', H, W, lambda: _ramp(H, W))
        add('zeros', H, W, lambda: np.zeros(H * (W + 1), np.uint8))
        add('noise', H, W, lambda: _noise_without_runs(H, W, rng), n_img=3 if (H, W) == (3, 64) else 1)
        add('fish', H, W, lambda: _fish(H, W, rng), n_img=3 if (H, W) == (33, 200) else 1)
        add('speckle', H, W, lambda: _speckle(H, W, rng), n_img=3 if (H, W) in ((5, 127), (70, 255)) else 1)
    for H, W in RAMP_EXTENTS:
        add('ramp', H, W, lambda: _ramp(H, W))
    # all zeros, plain and inverted, as PIXELS (the stream of the inverted one starts every line with 255)
    cases.append(('zero_pixels_40x90', np.zeros((1, 40, 90, 3), np.uint8), 1, 0))
    cases.append(('zero_pixels_inverted_40x90', np.zeros((1, 40, 90, 3), np.uint8), 0, 1))
    for R in PLACED_LENGTHS:
        for border in PLACED_BORDERS:
            for placement in PLACEMENTS:
                if placed_run(R, border, placement) is not None:
                    add('run%d_%s_%s' % (R, border, placement), *PLACED_EXTENT, lambda: _placed_stream(R, border, placement))
    add('fibonacci', 3, 900, lambda: _fibonacci(3, 900))
    return cases


CASES = build_cases()
IDS = [c[0] for c in CASES]
