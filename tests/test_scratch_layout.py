"""The drivers' scratch layouts (csrc/scratch.h, the *_bufs functions of csrc/common.h) checked on the CPU: tests/scratch_layout_check.cpp
is built with the host compiler under ASan + UBSan and run; it makes no HIP call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_places_what_it_measures_and_keeps_the_sizes(tmp_path):
    """For every layout function and the shapes 1 x 1, 33 x 70 and 1040 x 1392: the measuring and the placing pass give identical
    offsets, every slot is 256-byte aligned, inside the measured total and disjoint from the others, and as long as the buffer's own
    allocation was before the arenas."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    hip_inc = next((d for d in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include'), '/opt/rocm/include')
                    if os.path.exists(os.path.join(d, 'hip', 'hip_runtime.h'))), None)
    if hip_inc is None:
        pytest.skip('no HIP headers')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, timeout=120).returncode != 0:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    exe = str(tmp_path / 'scratch_layout_check')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + san + ['-D__HIP_PLATFORM_AMD__', '-isystem', hip_inc,
           os.path.join(ROOT, 'tests', 'scratch_layout_check.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'scratch_layout ok' in run.stdout
