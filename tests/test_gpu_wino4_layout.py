"""Bit-identity of the F(4x4) kernels across a change of their LDS layout (csrc/wino4_lds_layout.h): the layout decides where a value is
parked in LDS, never what is computed, so every output keeps its bits.  Single layers at the smallest shapes that reach every arm, under
`winograd` 2 (conv_wino4r_kernel, conv_wino4_kernel) and 3 (conv_wino4s_kernel where Cout % 64 == 0), with ReLU, linear and tanh:

    odd_regions   3 x 16 x 16, 8 -> 64      one 8-channel group, 3 regions: an odd count, the last workgroup's pair half empty
    tail4         2 x 32 x 48, 12 -> 64     Cin % 8 == 4: the upper channel half of the last group reads zeros
    cout96        2 x 32 x 32, 64 -> 96     Cout % 64 == 32: the second block's missing channel half
    split_k       2 x 32 x 32, 64 -> 32     conv_wino4_kernel (split-K, a lone 32-channel block)
    pool          2 x 32 x 32, 24 -> 64     fused 2x2 max-pool, three groups
    head          2 x 32 x 32, 16 -> 64     fused 4-class 1x1 softmax head (HEAD kernels, wino4_combine.inc's channel-half passes)
    crop          one 300 x 462 image through the cropped plan of a base-64 depth-1 U-Net: region lists (p.lut) and input boxes (in_box)

SHA-256 of each output against tests/golden/wino4_layer_digests.json, which tools/wino4_layer_digests.py --write recorded on an MI355X
from a build of the commit before the layout changed."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import wino4_layer_digests as wd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'wino4_layer_digests.json')) as f:
        return json.load(f)['digests']


def test_golden_file_lists_every_case(golden):
    assert sorted(golden) == sorted(wd.all_keys())


@pytest.mark.parametrize('key', wd.all_keys())
def test_f4x4_layer_keeps_its_bits(gpu, golden, key):
    assert wd.digest(gpu, key) == golden[key], key
