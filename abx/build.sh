#!/bin/bash
# abx/build.sh NAME [extra hipcc flags...]: build mp3_amd/csrc as build_ab/NAME.so (A/B experiments)
set -e
exec python3 -c '
import sys
sys.path.insert(0, ".")
from mp3_amd import _build
name, flags = sys.argv[1], sys.argv[2:]
_build.compile_hip("mp3_amd/csrc", "build_ab/%s.so" % name, "build_ab/obj/" + name, extra=flags)
' "$@"
