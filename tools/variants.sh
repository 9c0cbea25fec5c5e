#!/bin/bash
# Developer A/B: build libevstore_hip variants with extra -D flags for ONE source file (default evs_fused), or for several joined by '+'.
# usage: tools/variants.sh name1:"-DFLAG ..." name2@evs_cache:"-DFLAG" name3@evs_fused_rf+evs_fused_rf_lean:"-DFLAG"
#        ->  ev-store-dlrm_amd/lib/var/libevstore_hip_<name>.so
# The lean fused entry's build-time A/B:  nolean@evs_fused_rf_lean:"-DEVS_RF_LEAN=0"  nopre@evs_fused_rf_lean:"-DEVS_RF_LEAN_PRELOAD=0"
set -e
cd "$(dirname "$0")/../ev-store-dlrm_amd/csrc"
make -s
mkdir -p ../lib/var
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -I../../include"
for spec in "$@"; do
  nf="${spec%%:*}"; defs="${spec#*:}"
  name="${nf%%@*}"; files="evs_fused"; [[ "$nf" == *@* ]] && files="${nf#*@}"
  objs=$(ls ../lib/obj/*.o)
  for file in ${files//+/ }; do
    extra=""; [[ "$file" == evs_fused_rf_lean ]] && extra="-mllvm -amdgpu-kernarg-preload-count=14"   # (as csrc/Makefile: this unit only)
    /opt/rocm/bin/hipcc $FLAGS $extra $defs -c $file.hip -o ../lib/var/${file}_$name.o
    objs="$(echo "$objs" | grep -v "/$file.o") ../lib/var/${file}_$name.o"
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/var/libevstore_hip_$name.so $objs -lpthread
  echo built $name
done
