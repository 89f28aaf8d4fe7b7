# Build rsl_rl_amd/lib/variants/<name>/librslrl_amd.so: the in-tree objects with <unit>.o rebuilt from
# rsl_rl_amd/csrc/<unit>.hip with [extra hipcc flags] (A/B of one kernel file; never shipped).  `make` first.
#   scripts/build_variant.sh <name> <unit>[,<unit>...] [extra hipcc flags]
# A build knob of a shared header wants every unit that includes it: mlp_gemm,mlp_heads for mlp_gemm_x6.h
# (RSLRL_X6_DEPTH, RSLRL_H3_DEPTH, RSLRL_B_FIRST); RSLRL_W4_DEPTH / RSLRL_W8_DEPTH are mlp_gemm's, RSLRL_OUTBWD_U
# mlp_out_bwd's.
set -e
name=$1; units=$(echo "$2" | tr ',' ' '); shift 2
d=rsl_rl_amd/lib/variants/$name
mkdir -p $d/obj
objs=$(ls rsl_rl_amd/lib/obj/*.o)
for src in $units; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mcode-object-version=5 -Iinclude -Irsl_rl_amd/csrc "$@" -c rsl_rl_amd/csrc/$src.hip -o $d/obj/$src.o
  objs="$(echo $objs | tr ' ' '\n' | grep -v "/$src.o") $d/obj/$src.o"
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $d/librslrl_amd.so $objs -Wl,-rpath,/opt/rocm/lib -Wl,-soname,librslrl_amd.so
