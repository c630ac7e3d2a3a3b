#!/usr/bin/env python3
"""sha256 of the gfx950 code object of every unit of libphip.so and of the debug unit: the proof that a refactor left the device code alone.
Run it at the parent and at the head and compare the two listings.

    python tools/device_hashes.py [-DNAME=VALUE ...] [OBJECT ...]

Every unit of _ffi.UNITS and _ffi.DEBUG_UNIT is compiled device-only with the product's flags (HIPCC_FLAGS without -shared, the unit's own, a fixed build id
for phip.hip) plus --cuda-device-only -fuse-cuid=none, so that the object depends on the sources alone and not on where the tree lies.  Flags given on the
command line are added to every unit (-DMEGA_PROFILE=1, a test variant's flags); object names (phip_mega.o ...) restrict the listing to those units."""
import concurrent.futures
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mitsuba_amd import _ffi


def main(argv):
    extra = [a for a in argv if a.startswith("-")]
    only = [a for a in argv if not a.startswith("-")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in _ffi.HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-fuse-cuid=none"] + extra
    units = [u for u in _ffi.UNITS + [_ffi.DEBUG_UNIT] if not only or u[2] in only]
    with tempfile.TemporaryDirectory() as tmp:
        def run(unit):
            src, unit_flags, obj = unit
            build_id = ['-DPHIP_BUILD_ID="0000000000000000"'] if src == "phip.hip" else []
            out = os.path.join(tmp, obj)
            r = subprocess.run([hipcc] + flags + unit_flags + build_id + ["-c", os.path.join(_ffi.CSRC, src), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed for %s:\n%s" % (obj, r.stdout))
            with open(out, "rb") as f:
                return obj, hashlib.sha256(f.read()).hexdigest()
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
            for obj, digest in pool.map(run, units):
                print("%-20s %s" % (obj, digest))


if __name__ == "__main__":
    main(sys.argv[1:])
