#!/bin/bash
# scratch/so/lib_<name>.so: the library with resnet.hip rebuilt with extra defines: build_resnet_variant.sh name [-Dxxx ...]; run with ICL_SO_PATH=scratch/so/lib_<name>.so
name=$1; shift
mkdir -p /root/repo/scratch/so
cd /root/repo/imageclust_amd/csrc && make -s >/dev/null 2>&1
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable -I../../include "$@" -c resnet.hip -o /tmp/resnet_$name.o 2>&1 | grep -E "error"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o ../../scratch/so/lib_$name.so $(ls *.o | grep -v "^resnet\.o$") /tmp/resnet_$name.o && ls -la ../../scratch/so/lib_$name.so
