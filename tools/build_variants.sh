#!/bin/bash
# Side builds of the library for A/B timing through ECSEG_HIP_LIB (other objects are reused from the product build):
#   diag            ecseg_amd/libecseg_diag.so with -DECSEG_DIAG: the in-kernel cycle stamps of conv_wino16_kernel
#                   (tools/w16_stamp_probe.py, read back through ecseg_debug_peek) exist only there
#   points12        ecseg_amd/libecseg_points12.so: the three F(4x4) kernels with the textbook interpolation points {0, +-1, +-2, inf}
#   <name>:<flags>  wino4_kernel.hip (the split-K kernel of the Cout = 32 layers) AND the host files with <flags> -> ecseg_amd/libecseg_v<name>.so
# Of the host files, ECSEG_DIAG concerns api.hip (ecseg_debug_peek) and the point pair filter_layout.hip (winograd4_filter): those are compiled
# with the flag, the product objects are linked for the rest.
#   <flag>          anything else is passed as -D<flag> to wino4_kernel.hip only (e.g. ECSEG_W4_TSLOTS=2) -> ecseg_amd/libecseg_v<flag>.so
set -e
cd "$(dirname "$0")/../ecseg_amd/csrc"
mkdir -p /tmp/w4
HC="/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC"
HOSTSRC="api filter_layout model_load plan_run segment drivers_post drivers_interseg drivers_fish drivers_files drivers_nuset"
for v in "$@"; do
  if [ "$v" = diag ]; then
    $HC -DECSEG_DIAG -c api.hip -o /tmp/w4/api_diag.o &
    $HC -DECSEG_DIAG -c wino16_kernel.hip -o /tmp/w4/wino16_diag.o &
  elif [ "$v" = points12 ]; then
    for k in wino4 wino4r wino4s; do $HC -fno-slp-vectorize -DECSEG_W4_PA=1 -DECSEG_W4_PB=2 -c ${k}_kernel.hip -o /tmp/w4/${k}_p12.o & done
    $HC -DECSEG_W4_PA=1 -DECSEG_W4_PB=2 -c filter_layout.hip -o /tmp/w4/filter_layout_p12.o &
  elif [[ "$v" == *:* ]]; then
    n=${v%%:*}; f=${v#*:}
    $HC -fno-slp-vectorize $f -c wino4_kernel.hip -o /tmp/w4/wino4_v$n.o &
    for k in $HOSTSRC; do $HC $f -c $k.hip -o /tmp/w4/${k}_v$n.o & done
  else
    $HC -fno-slp-vectorize -D$v -c wino4_kernel.hip -o /tmp/w4/wino4_v$v.o &
  fi
done
wait
LK="/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC"
HOST="model_load.o plan_run.o segment.o drivers_post.o drivers_interseg.o drivers_fish.o drivers_files.o drivers_nuset.o"   # host objects no variant flag concerns
REST="layer_kernels.o convs_kernel.o ccl_kernels.o meta_inference_kernels.o overlay_kernels.o stitch_preprocess_kernels.o interseg_kernels.o fishdist_kernels.o host_codec.o host_io.o comm.o -lz -ldl"   # objects of the product build
W4RS="wino4r_kernel.o wino4s_kernel.o"
for v in "$@"; do
  if [ "$v" = diag ]; then
    $LK -o ../libecseg_diag.so /tmp/w4/api_diag.o filter_layout.o $HOST unet_kernels.o wino4_kernel.o /tmp/w4/wino16_diag.o $W4RS $REST
  elif [ "$v" = points12 ]; then
    $LK -o ../libecseg_points12.so api.o /tmp/w4/filter_layout_p12.o $HOST unet_kernels.o /tmp/w4/wino4_p12.o /tmp/w4/wino4r_p12.o /tmp/w4/wino4s_p12.o wino16_kernel.o $REST
  elif [[ "$v" == *:* ]]; then
    n=${v%%:*}
    $LK -o ../libecseg_v$n.so $(for k in $HOSTSRC; do echo /tmp/w4/${k}_v$n.o; done) unet_kernels.o /tmp/w4/wino4_v$n.o wino16_kernel.o $W4RS $REST
  else
    $LK -o ../libecseg_v$v.so api.o filter_layout.o $HOST unet_kernels.o /tmp/w4/wino4_v$v.o wino16_kernel.o $W4RS $REST
  fi
done
ls -la ../libecseg_*.so
