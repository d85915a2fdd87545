#!/bin/bash
# Build a diagnostic VARIANT of libeae.so beside the product library (which stays untouched):
#   tools/build_variant.sh stamps -DEAE_STAMPS        -> <pkg>/libeae_stamps.so   (use with EAE_LIB_PATH=<that file>)
set -e
TAG=$1; shift
PKG=$(dirname "$0")/../hybrid-autoencoder-mlp-pipeline-for-satellite-image-classification_amd
PKG=$(cd "$PKG" && pwd)
OBJ=$PKG/csrc/_obj_$TAG
mkdir -p "$OBJ"
# the translation units are the product library's (build.SOURCES)
SOURCES=$(cd "$PKG" && python3 -c "import build; print(' '.join(s[:-len('.hip')] for s in build.SOURCES))")
pids=(); objs=()
for s in $SOURCES; do
  hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-result "$@" -c "$PKG/csrc/$s.hip" -o "$OBJ/$s.o" &
  pids+=($!); objs+=("$OBJ/$s.o")
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$PKG/libeae_$TAG.so" "${objs[@]}"
echo "$PKG/libeae_$TAG.so"
