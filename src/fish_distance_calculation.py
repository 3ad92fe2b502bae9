#!/usr/bin/env python3
# `make fish_distance_calculation` entry point with the reference's path; the implementation is ecseg_amd/fish_distance_calculation.py.
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecseg_amd.fish_distance_calculation import main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1:])
