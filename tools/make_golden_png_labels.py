"""Records tests/golden/png_labels_sha256.json: SHA-256 of the file ecseg_png_write_labels writes for every case of
tests/png_label_cases.py.  Run on the commit BEFORE deflate_labels was split (png_label_code.h): the test holds every later
host coder, and through it the device coder, to these bytes.  ``python -m tools.make_golden_png_labels``."""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import png_label_cases as pc
    from ecseg_amd import image_io
    out = {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'l.png')
        for c in pc.CASES:
            image_io.write_label_png(path, c.labels)
            out[c.name] = hashlib.sha256(open(path, 'rb').read()).hexdigest()
    with open(os.path.join(ROOT, 'tests', 'golden', 'png_labels_sha256.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(len(out), 'cases')


if __name__ == '__main__':
    main()
