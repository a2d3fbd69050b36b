#!/bin/bash
# Builds lib/variants/librt_hip_NAME.so from the device sources of git revision REV (the current
# host objects), for interleaved A/B runs against the working tree (tools/ab.sh, ab_frame.py) --
# dev tool, CPU side.   usage: tools/build_ab.sh REV NAME [extra hipcc flags]
# The whole of csrc/device is taken from REV, so rt_render.hip's .inc and .hpp includes are REV's
# too.  It is unpacked into a temporary tree of the repository's shape that gets the working tree's
# include/ (a link) and csrc/host headers (copies, so that their "../device/" resolves to REV's):
# the public headers and the host builders that lib/device_image.o was built from.
set -e -o pipefail
REV=${1:?rev}; NAME=${2:?name}; shift 2
cd "$(dirname "$0")/.."
ROOT=$PWD
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
git archive "$REV" my-raytracer_amd/csrc/device | tar -x -C "$TMP"
ln -s "$ROOT/include" "$TMP/include"
mkdir "$TMP/my-raytracer_amd/csrc/host"
cp "$ROOT"/my-raytracer_amd/csrc/host/*.hpp "$TMP/my-raytracer_amd/csrc/host/"
cd my-raytracer_amd
make -s lib/device_image.o
make -s variant HIP_SRC="$TMP/my-raytracer_amd/csrc/device/rt_render.hip" N="$NAME" V="$*"
ls -la "lib/variants/librt_hip_$NAME.so"
