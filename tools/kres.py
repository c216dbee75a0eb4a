"""Per-kernel register use of the decode kernels' translation units
(hipcc -Rpass-analysis=kernel-resource-usage):
    python tools/kres.py [filter]
A filter that names one family (rs_kernel, ro_kernel, sp_kernel, decode_kernel) compiles only
that family's file."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(__file__).rsplit("/tools/", 1)[0]
flt = sys.argv[1] if len(sys.argv) > 1 else "rs_kernel"
FAMILY = {"rs_kernel": "gpd_rs.hip", "ro_kernel": "gpd_ro.hip", "sp_kernel": "gpd_sp.hip",
          "decode_kernel": "gpd_kernels.hip"}  # (gopacket_amd.build KERNEL_SOURCES)
srcs = [os.path.join(ROOT, "gopacket_amd", "csrc", f) for f in ([FAMILY[flt]] if flt in FAMILY else FAMILY.values())]


def remarks(src):
    with tempfile.TemporaryDirectory() as d:
        return subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", ROOT + "/include",
                               "-c", src, "-o", os.path.join(d, "kres.o")] + os.environ.get("GPD_EXTRA_CFLAGS", "").split() +
                              ["-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr


with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
    text = "".join(ex.map(remarks, srcs))
cur, rows = None, []
for line in text.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        rows.append(cur)
        continue
    m = re.search(r"(VGPRs|VGPRs Spill|Occupancy \[waves/SIMD\]|AGPRs|LDS Size \[bytes/block\]): (\d+)", line)
    if m and cur is not None:
        cur[m.group(1)] = int(m.group(2))
for c in rows:
    if flt in c["name"]:
        print(f"{c.get('VGPRs', '?'):>4} vgpr {c.get('VGPRs Spill', 0):>3} spill occ {c.get('Occupancy [waves/SIMD]', '?')}  {c['name']}")
