#!/bin/bash
# Builds compu_amd/libcompu_hip.so for gfx950 (cross-compiles without a GPU).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../libcompu_hip.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# the brotli static dictionary (RFC 7932 Appendix A) becomes a device array: brotli.hip includes build/brotli_dict.inc
mkdir -p "$here/build"
python3 - "$here/brotli_dict.bin" "$here/build/brotli_dict.inc" <<'PY'
import hashlib, sys
data = open(sys.argv[1], "rb").read()
want = "20e42eb1b511c21806d4d227d07e5dd06877d8ce7b3a817f378f313653f35c70"
if len(data) != 122784 or hashlib.sha256(data).hexdigest() != want:
    sys.exit("brotli_dict.bin is not the RFC 7932 dictionary")
with open(sys.argv[2], "w") as f:
    for i in range(0, len(data), 32):
        f.write(",".join(str(x) for x in data[i:i + 32]) + ",\n")
PY
"$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall \
    -o "$out" "$here"/*.hip "$@"
echo "built $out"
if [ "${CHIP_BUILD_STATS:-0}" = "1" ]; then
    "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -DCHIP_STATS \
        -o "$here/../libcompu_hip_stats.so" "$here"/*.hip
    echo "built $here/../libcompu_hip_stats.so (diagnostic)"
    # the same with literal pairing compiled out of the inflate walk: the yardstick of tests/test_inflate_pairs_gpu.py's super-round count
    "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -DCHIP_STATS -DCHIP_EXP_NO_PAIR \
        -o "$here/../libcompu_hip_stats_nopair.so" "$here"/*.hip
    echo "built $here/../libcompu_hip_stats_nopair.so (diagnostic)"
fi
# C++ replay of the reference's integration tests over the C ABI (runs on the GPU box only)
g++ -O1 -std=c++17 -Wall -o "$here/../../tests/cpp/test_reference" "$here/../../tests/cpp/test_reference.cpp" \
    -L"$here/.." -lcompu_hip -Wl,-rpath,'$ORIGIN/../../compu_amd' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64
echo "built tests/cpp/test_reference"
