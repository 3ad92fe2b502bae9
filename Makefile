.PHONY: build metaseg meta_overlay interseg stat_fish fish_distance_calculation test asan clean

# same targets and config.yaml surface as the reference (Makefile:6-10); `build` compiles the gfx950 library first
build:
	python -m ecseg_amd.build

metaseg: build
	python src/metaseg.py

meta_overlay: build
	python src/meta_overlay.py

interseg: build
	python src/interseg.py

stat_fish: build
	python src/stat_fish.py

fish_distance_calculation: build
	python src/fish_distance_calculation.py

test:
	python -m pytest tests -q -m "not gpu"

# AddressSanitizer + UBSan build of the host-side codecs (the only code that parses untrusted bytes) with a corrupt-stream
# corpus; CPU only (GPU sanitizers are not available on the target pool)
asan:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp ecseg_amd/csrc/host_io.cpp tools/asan/codec_fuzz.cpp -lz -o /tmp/ecseg_codec_fuzz
	/tmp/ecseg_codec_fuzz

# the same for the device TIFF reader: its per-strip routine (csrc/tiff_decode_strip.h) compiled for the host, lanes as a loop, against
# the host decoder on built-in streams; tests/test_tiff_decode.py runs it on the tests' corpus too
.PHONY: asan_tiff_decode
asan_tiff_decode:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp tools/asan/tiff_decode_fuzz.cpp -o /tmp/ecseg_tiff_decode_fuzz
	/tmp/ecseg_tiff_decode_fuzz

# and for its Deflate strips: the per-strip routine (csrc/tiff_inflate_strip.h) compiled for the host, lanes as a loop, against the
# host reader's rule made of the same zlib calls, on built-in streams, seeded valid streams and seeded mutations;
# tests/test_tiff_inflate.py builds and runs it on the tests' corpus too
.PHONY: asan_tiff_inflate
asan_tiff_inflate:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/tiff_inflate_fuzz.cpp -lz -o /tmp/ecseg_tiff_inflate_fuzz
	/tmp/ecseg_tiff_inflate_fuzz

# and for its PackBits strips (csrc/tiff_packbits_strip.h, the body of tiffb_packbits_kernel): seeded valid, truncated and overlong
# streams against a plain byte loop that restates image_io._packbits_decode; tests/test_tiff_packbits.py builds and runs it
.PHONY: asan_tiff_packbits
asan_tiff_packbits:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/tiff_packbits_fuzz.cpp -o /tmp/ecseg_tiff_packbits_fuzz
	/tmp/ecseg_tiff_packbits_fuzz

# and for the batched reader: the layout function (csrc/tiff_decode_batch.h) and the batched strip walk over packed batches with
# corrupt and truncated files; tests/test_tiff_decode_batch.py builds and runs it
.PHONY: asan_tiff_decode_batch
asan_tiff_decode_batch:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp tools/asan/tiff_decode_batch_fuzz.cpp -o /tmp/ecseg_tiff_decode_batch_fuzz
	/tmp/ecseg_tiff_decode_batch_fuzz

# and for its tiled files (option tiff_tiled_on_device): the tile-table parse, tile_place (csrc/tiff_parse.h), the layout with staging
# slots and the staging -> raster walk of tiffb_untile_kernel (csrc/tiff_untile.h) compiled for the host, lanes as a loop, against a
# naive untile; tests/test_tiff_tiles.py builds and runs it.  TIFF_TILES_CHECK: where the program is put
TIFF_TILES_CHECK ?= /tmp/ecseg_tiff_tiles_check
.PHONY: asan_tiff_tiles
asan_tiff_tiles:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp ecseg_amd/csrc/host_io.cpp tools/asan/tiff_tiles_check.cpp -lz -o $(TIFF_TILES_CHECK)
	$(TIFF_TILES_CHECK)

# and for the batched writer: the layout function (csrc/tiff_encode_batch.h) over seeded file lists and the strip routine of the
# encode kernels (csrc/tiff_encode_strip.h) compiled for the host, lanes as a loop, against the host encoder;
# tests/test_tiff_encode_batch.py builds and runs it
.PHONY: asan_tiff_encode_batch
asan_tiff_encode_batch:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp tools/asan/tiff_encode_batch_fuzz.cpp -o /tmp/ecseg_tiff_encode_batch_fuzz
	/tmp/ecseg_tiff_encode_batch_fuzz

# and for the device gray PNG coder: the per-block pieces of its kernels (csrc/png_gray_tokens.h) and the host parts of its code
# (csrc/png_gray_code.h) walked as the kernels walk them, against rle_scan and the host writer's file; tests/test_png_gray.py builds
# and runs it
.PHONY: asan_png_gray
asan_png_gray:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    ecseg_amd/csrc/host_codec.cpp ecseg_amd/csrc/host_io.cpp tools/asan/png_gray_fuzz.cpp -lz -o /tmp/ecseg_png_gray_fuzz
	/tmp/ecseg_png_gray_fuzz

# and for interSeg's classifiers on the device: the per-element function of the ecSeg-c input and the selection and chunk planning
# of ecseg_classify_nucleus_crops (csrc/iseg_classify.h, the text the kernel and the driver compile); tests/test_iseg_classify.py
# builds and runs it, and holds its output to numpy and to classify_crops' rules.  ISEG_CHECK: where the program is put
ISEG_CHECK ?= /tmp/ecseg_iseg_classify_check
.PHONY: asan_iseg_classify
asan_iseg_classify:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/iseg_classify_check.cpp -o $(ISEG_CHECK)
	$(ISEG_CHECK)

# and for interseg.batch: the planning header of ecseg_interseg_batch (csrc/iseg_batch.h) - table, groups, capacities, crop windows
# and chunk runs - over layouts with gaps, reversed order, zero-nucleus images and capacities one short;
# tests/test_interseg_batch.py builds and runs it.  ISEG_BATCH_CHECK: where the program is put
ISEG_BATCH_CHECK ?= /tmp/ecseg_iseg_batch_check
.PHONY: asan_iseg_batch
asan_iseg_batch:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/iseg_batch_check.cpp -o $(ISEG_BATCH_CHECK)
	$(ISEG_BATCH_CHECK)

# and for stat_fish.batch: the layout header of ecseg_stat_fish_batch (csrc/fish_batch.h) - rasters, typed arrays by element, padded
# planes, the arena and its restated byte count - over seeded chunks, reversed order, mixed C and K, zero-nucleus images and capacities
# one short; tests/test_stat_fish_batch.py builds and runs it.  FISH_BATCH_CHECK: where the program is put
FISH_BATCH_CHECK ?= /tmp/ecseg_fish_batch_check
.PHONY: asan_fish_batch
asan_fish_batch:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/fish_batch_check.cpp -o $(FISH_BATCH_CHECK)
	$(FISH_BATCH_CHECK)

# and for ecseg_min_cut_regions: the layout header (csrc/mincut_regions.h) - selection, windows, centre records, capacities and the
# arena - over seeded label lists, zero regions and capacities one short; tests/test_min_cut_regions.py builds and runs it.
# MIN_CUT_REGIONS_CHECK: where the program is put
MIN_CUT_REGIONS_CHECK ?= /tmp/ecseg_min_cut_regions_check
.PHONY: asan_min_cut_regions
asan_min_cut_regions:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/min_cut_regions_check.cpp -o $(MIN_CUT_REGIONS_CHECK)
	$(MIN_CUT_REGIONS_CHECK)

# and for fish_distance_calculation.batch: the layout header of ecseg_fish_distances_batch (csrc/fishdist_batch.h) - the global pixel
# axis, the runs of tiles and blocks with their lookup, the two-part buffer, the groups and the limits - over seeded shape lists with
# extents of 1 and ragged tiles; tests/test_fish_distance_batch.py builds and runs it.  FISHDIST_BATCH_CHECK: where the program is put
FISHDIST_BATCH_CHECK ?= /tmp/ecseg_fishdist_batch_check
.PHONY: asan_fishdist_batch
asan_fishdist_batch:
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
	    tools/asan/fishdist_batch_check.cpp -o $(FISHDIST_BATCH_CHECK)
	$(FISHDIST_BATCH_CHECK)

clean:
	rm -rf __pycache__ ecseg_amd/csrc/*.o ecseg_amd/libecseg_*.so
