"""The LDS layout of the F(4x4) kernels (csrc/wino4_lds_layout.h) against the bank rule of the LDS, on the CPU: tools/lds_bank_model.cpp is
built with the host compiler - it includes the header the kernels include, makes no HIP call and needs no GPU - and walks the 768
threads of a workgroup through every LDS access site of conv_wino4r_kernel, conv_wino4s_kernel and conv_wino4_kernel.

Instruction per site, as read in the disassembly of the product build (hipcc -O3 --offload-arch=gfx950 -fno-slp-vectorize; the source
type alone would say ds_read_b64 / ds_write_b32 for several of them):
    row_pass raw reads        ds_read2_b64 (raw rows 0|1, 2|3, 4|5)      two accesses, 4 x 16 contiguous lanes, bank (a / 4) % 32
    row_pass t-image writes   ds_write_b64                               4 x 16 contiguous lanes, (a / 4) % 32
    load_t column reads       ds_read_b128                               4 x 16 lanes {0-3,12-15,20-27} ..., (a / 4) % 64
    filter-stage reads        ds_read_b128 (fp32 kernels, split kernel), ds_read_b64 (split kernel's u3: 2 x 32 lanes, (a / 4) % 64)
    fold writes               ds_write2_b32 / ds_write2st64_b32          two ds_write_b32: 2 x 32 lanes, (a / 4) % 32
    adding folds' reads       ds_read2_b32                               two ds_read_b32: 2 x 32 lanes, (a / 4) % 32
    combine reads             ds_read_b128
    split-K ring reads        ds_read_b64 and ds_read2_b64
Identical addresses broadcast, lanes >= 48 of row_pass are inactive, every further distinct address on a busy bank of a lane group costs
one cycle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sites the layout can place freely: each must sit at the minimum of its instruction
FREE_SITES = {'row_pass.raw_read', 'row_pass.t_write', 'load_t.t_read', 'filter.read_fp32', 'filter.read_split16', 'filter.read_split8', 'fold.write',
              'fold.write_tile_half', 'fold.add_read', 'combine.read', 'combine.read_tile_half'}
# the split-K kernel reads 8 of the 16 bytes of a slot per lane and the slot is the LDS-DMA's granule: one cycle per lane group is lost under
# any placement (tools/lds_bank_model.cpp, Site::floor); the layout must lose no more than that
FLOOR_SITES = {'split_k.ring_read', 'split_k.ring_read_paired'}


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('lds_bank_model') / 'lds_bank_model')
    out = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'ecseg_amd', 'csrc'),
                          os.path.join(ROOT, 'tools', 'lds_bank_model.cpp'), '-o', exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    res = {'parent': {}, 'new': {}}
    for line in run.stdout.splitlines():
        f = line.split()
        if f[1] == 'total':
            continue
        res[f[0]][f[1]] = dict(inst=f[2], **{f[i]: int(f[i + 1]) for i in range(3, len(f), 2)})
    print(run.stdout)
    return res


def test_model_lists_every_site_in_both_layouts(model):
    for layout in ('parent', 'new'):
        assert set(model[layout]) == FREE_SITES | FLOOR_SITES, layout
        assert all(s['insts'] > 0 and s['min'] > 0 for s in model[layout].values())


def test_model_sees_the_conflicts_of_the_layout_before_round_9(model):
    """The frozen layout of the commit before: two-way conflicts in the row pass - three extra cycles per ds_write_b64 (every 16-lane group
    puts two of its eight slots on the banks of two others) and one per straddling pair read."""
    extra = {k: v['extra'] - v['floor'] for k, v in model['parent'].items()}
    assert extra['row_pass.t_write'] == 3 * model['parent']['row_pass.t_write']['insts']
    assert extra['row_pass.raw_read'] > 0
    assert all(v == 0 for k, v in extra.items() if not k.startswith('row_pass.'))


def test_every_site_of_the_current_layout_is_at_its_minimum(model):
    for k in sorted(FREE_SITES):
        assert model['new'][k]['extra'] == 0 and model['new'][k]['floor'] == 0, (k, model['new'][k])
    for k in sorted(FLOOR_SITES):
        assert model['new'][k]['extra'] == model['new'][k]['floor'], (k, model['new'][k])
