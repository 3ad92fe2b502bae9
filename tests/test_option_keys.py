"""Every key of ecseg_set_option (csrc/api.hip) is set by a GPU test and documented: the keys are parsed from the function's
``k == "..."`` comparisons; each must appear as ``set_option('<key>'`` in a tests/test_gpu_*.py, and the option table of INTEGRATION.md
must list exactly these keys.  An option nobody sets is a path nobody runs."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key -> why no GPU test sets it.  One key at most: crop_mask.
EXEMPT = {
    'crop_mask': 'with 0 the last bits of the result depend on what the buffers held before, by design (csrc/ctx.h: crop_mask; '
                 'INTEGRATION.md: "0 only for A/B timing"), so no exact test of that value exists',
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding='utf-8') as f:
        return f.read()


def option_keys():
    """The keys ecseg_set_option compares its argument with, in the order of the source."""
    src = _read('ecseg_amd', 'csrc', 'api.hip')
    start = src.index('int ecseg_set_option(')
    body = src[start:src.index('\n}\n', start)]
    keys = re.findall(r'\bk == "([^"]+)"', body)
    assert len(keys) == len(set(keys)), keys
    return keys


def keys_set_by_gpu_tests():
    """key -> the GPU test files with a literal ``set_option('<key>'`` call"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'test_gpu_*.py'))):
        with open(path, encoding='utf-8') as f:
            text = f.read()
        if 'pytest.mark.gpu' not in text:
            continue
        for key in re.findall(r'''set_option\(\s*['"]([A-Za-z0-9_]+)['"]''', text):
            found.setdefault(key, []).append(os.path.basename(path))
    return found


def documented_keys():
    """The first column of the table under ``ecseg_set_option(h, key, value)`` in INTEGRATION.md"""
    lines = _read('INTEGRATION.md').split('\n')
    at = [i for i, line in enumerate(lines) if line.startswith('`ecseg_set_option(h, key, value)`')]
    assert len(at) == 1, 'INTEGRATION.md: one paragraph opens the option table'
    i = at[0] + 1
    while not lines[i].startswith('|'):
        assert not lines[i].strip(), lines[i]
        i += 1
    assert [c.strip() for c in lines[i].strip('|').split('|')] == ['key', 'default', 'meaning'] and set(lines[i + 1]) <= set('|-')
    keys = []
    for line in lines[i + 2:]:
        if not line.startswith('|'):
            break
        m = re.match(r'\| `([a-z0-9_]+)` \|', line)
        assert m, line
        keys.append(m.group(1))
    return keys


def test_the_parser_finds_the_options():
    keys = option_keys()
    assert len(keys) >= 18, keys
    for known in ('overlap_post', 'post_chunk', 'images_per_group', 'unet_lanes', 'lane_auto_windows', 'blocking_wait', 'winograd', 'crop_mask'):
        assert known in keys, known


def test_every_option_is_set_by_a_gpu_test():
    assert set(EXEMPT) <= {'crop_mask'} and all(len(why) > 40 for why in EXEMPT.values())
    keys, found = option_keys(), keys_set_by_gpu_tests()
    assert not set(EXEMPT) - set(keys), 'an exemption for a key that is gone'
    missing = [k for k in keys if k not in found and k not in EXEMPT]
    assert not missing, 'no tests/test_gpu_*.py sets %s' % missing
    unknown = sorted(set(found) - set(keys))
    assert not unknown, 'GPU tests set %s, which ecseg_set_option does not know' % unknown


def test_the_option_table_lists_exactly_the_options():
    keys, doc = option_keys(), documented_keys()
    assert len(doc) == len(set(doc)), 'a key is listed twice'
    assert sorted(doc) == sorted(keys), 'undocumented: %s; documented but unknown: %s' % (sorted(set(keys) - set(doc)), sorted(set(doc) - set(keys)))
