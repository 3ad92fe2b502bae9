"""Every layout of the drivers' scratch arenas has a row in tests/test_gpu_scratch.py (no GPU).  The ``lay_out(`` call sites under
ecseg_amd/csrc are parsed for the layout functions they call (``*_bufs``, ``post_workspace``) and for buffers taken bare in the
lambda; each site - the function it stands in, its arena, its layouts - must stand in tests/scratch_drivers.py: SITE_ROWS, mapped to
rows the GPU module holds, or in EXEMPT with a reason.  A driver added later that lays out in an arena without a row fails here, also
when it reuses a layout function another driver has a row for."""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scratch_drivers as sd                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ecseg_amd', 'csrc')
# a definition at the left margin, of any return type: `static inline std::string name(`, `template <..> int name(` ...
FUNCTION = re.compile(r'^(?!\s|//|#|typedef|using|namespace|extern|struct|enum|return|if|for|while|else)[\w:<>,&*\s]+?[\s*&](\w+)\s*\([^;{]*\)\s*(?:const\s*)?\{', re.M)


def enclosing_function(text, at):
    """the last function defined at the left margin before ``at`` whose body - up to the first `}` at the left margin - holds ``at``"""
    found = None
    for m in FUNCTION.finditer(text, 0, at):
        found = m
    assert found, 'no function in front of the site'
    end = re.compile(r'^\}', re.M).search(text, found.end())
    assert end and end.start() > at, 'the site at %d lies behind the end of %s' % (at, found.group(1))
    return found.group(1)


def _call_text(text, at):
    """the text of the call that opens at ``at`` (the index of its opening bracket), brackets balanced"""
    depth = 0
    for k in range(at, len(text)):
        depth += text[k] == '('
        depth -= text[k] == ')'
        if depth == 0:
            return text[at:k + 1]
    raise AssertionError('unbalanced call')


def call_sites():
    """-> [(file, function the site stands in, arena, [layout names])] of every lay_out call under csrc (its definition left out)"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h'))):
        text = open(path).read()
        for m in re.finditer(r'\blay_out\(', text):
            if text[:m.start()].rstrip().endswith('int'):     # the template's own definition (ctx.h)
                continue
            call = _call_text(text, m.end() - 1)
            before = [enclosing_function(text, m.start())]
            arena = re.search(r'h->(\w+_arena)', call)
            assert arena, (path, call[:60])
            names = re.findall(r'\b(\w+_bufs|post_workspace)\s*\(', call)
            if re.search(r'\bc\.take<', call):
                names.append('take@' + before[-1])
            assert names, (path, before[-1], 'a lay_out call that lays nothing out?')
            out.append((os.path.basename(path), before[-1], arena.group(1), names))
    return out


def test_the_parser_finds_the_call_sites():
    sites = call_sites()
    assert len(sites) >= 36                                  # (36 when this test was written)
    assert {s[2] for s in sites} == {'post_arena', 'call_arena', 'count_arena', 'keep_arena', 'pre_arena'}
    assert ('segment.hip', 'ensure_post', 'post_arena', ['post_workspace']) in sites
    assert ('drivers_fish.hip', 'ecseg_min_cut_regions', 'count_arena', ['take@ecseg_min_cut_regions']) in sites
    both = [s for s in sites if s[1] == 'ecseg_fish_render_tiff']
    assert both and both[0][3] == ['fish_render_bufs', 'tiff_encode_bufs']


def test_every_call_site_has_a_row_or_a_reason():
    """keyed on the site - the function it stands in, the arena, the layouts - not on the layout's name: a driver that reuses an
    existing ``*_bufs`` function is a new site"""
    seen = {(fn, arena, tuple(names)) for _, fn, arena, names in call_sites()}
    missing = sorted(seen - set(sd.SITE_ROWS) - set(sd.EXEMPT))
    assert not missing, 'lay_out sites without a row in tests/scratch_drivers.py (add the driver to tests/test_gpu_scratch.py): %s' % missing
    stale = sorted((set(sd.SITE_ROWS) | set(sd.EXEMPT)) - seen)
    assert not stale, 'tests/scratch_drivers.py names sites that ecseg_amd/csrc does not hold: %s' % stale
    assert not set(sd.SITE_ROWS) & set(sd.EXEMPT)
    for site, why in sd.EXEMPT.items():
        assert isinstance(why, str) and len(why.split()) >= 5, 'EXEMPT[%r] needs a written reason' % (site,)


def test_a_new_driver_that_reuses_a_layout_fails_the_guard():
    seen = {(fn, arena, tuple(names)) for _, fn, arena, names in call_sites()}
    later = ('ecseg_some_later_driver', 'call_arena', ('tiff_encode_bufs',))
    assert later not in sd.SITE_ROWS and (seen | {later}) - set(sd.SITE_ROWS) - set(sd.EXEMPT) == {later}


def test_every_arena_is_laid_out_by_some_row():
    arenas = {site[1] for site, rows in sd.SITE_ROWS.items() if rows}
    assert arenas == {'post_arena', 'call_arena', 'count_arena', 'keep_arena', 'pre_arena'}


def test_every_row_named_is_a_driver_of_the_gpu_module():
    import test_gpu_scratch as gpu_module
    assert len(set(sd.ROWS)) == len(sd.ROWS)
    assert set(gpu_module.DRIVERS) == set(sd.ROWS)
    for site, rows in sd.SITE_ROWS.items():
        assert rows and set(rows) <= set(sd.ROWS), site
    assert set(sd.ROWS) == {r for rows in sd.SITE_ROWS.values() for r in rows}, 'a row that runs no layout'
