#!/bin/bash
# tools/ab_build.sh NAME "-DFOO=1 -DBAR=0"  -> hlynr_intercept_amd/libhlx_NAME.so (A/B experiments)
# the product's compile recipe (hlynr_intercept_amd/build.py, FLAGS) plus the given macros, as one translation unit;
# add -DHLX_AB_MINIMAL to compile only the base variant (bench.py's default workload): ~15 s instead of ~90 s
set -e
cd "$(dirname "$0")/.."
python3 -c 'import sys; from hlynr_intercept_amd import build; build.build_variant(sys.argv[1], sys.argv[2].split())' \
    "$PWD/hlynr_intercept_amd/libhlx_$1.so" "$2"
python3 tools/check_hot_words.py hlynr_intercept_amd/libhlx_$1.so   # refuse variants that spill a hot-word register
