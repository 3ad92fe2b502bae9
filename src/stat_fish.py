#!/usr/bin/env python3
# `make stat_fish` entry point with the reference's path; the implementation is ecseg_amd/stat_fish.py.
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecseg_amd.stat_fish import main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1:])
