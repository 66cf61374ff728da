#!/bin/bash
# per-kernel VGPR / AGPR / scratch / LDS of the built engine (reads the gfx950 code objects inside librabe_hip.so: the .hip_fatbin section holds
# one offload bundle per device translation unit, each is unbundled and listed in turn)
set -e
T=$(mktemp -d)
objcopy -O binary --only-section=.hip_fatbin "$(dirname "$0")/../rabe_amd/librabe_hip.so" $T/fat.bin
python3 - "$T" <<'PY'
import os, sys
T = sys.argv[1]
d = open(os.path.join(T, "fat.bin"), "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
starts = []
i = d.find(magic)
while i >= 0:
    starts.append(i)
    i = d.find(magic, i + 1)
for k, s in enumerate(starts):
    e = starts[k + 1] if k + 1 < len(starts) else len(d)
    open(os.path.join(T, "bundle%02d.bin" % k), "wb").write(d[s:e])
PY
for b in $T/bundle*.bin; do
  /opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$b --output=$b.o
  /opt/rocm/lib/llvm/bin/llvm-readelf --notes $b.o | python3 -c "
import sys, re
for b in sys.stdin.read().split('- .agpr_count')[1:]:
    g = lambda k: (re.search(k + r':\s+(\S+)', b) or [None, '?'])[1]
    print('%-28s agpr %-4s vgpr %-4s scratch %-6s lds %s' % (re.sub(r'^_Z\d+', '', g(r'\.name'))[:28], b.split()[1], g(r'\.vgpr_count'), g(r'\.private_segment_fixed_size'), g(r'\.group_segment_fixed_size')))
"
done
rm -rf $T
