#!/usr/bin/env python
"""Record tests/golden/beam_dispatch_parent.npz: every output word of the calls of tests/beam_dispatch_calls.py on ANOTHER commit's
library, on the MI355X, in a process of its own:

    timeout -k 10 300 python tools/dev/beam_dispatch_record.py --lib ../parent/policy_gradient_asr_amd/libpgasr_hip.so --commit <id>

Every call is made twice; the file is written only if no word differs between the two runs, so that it cannot encode run-to-run variation.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the library to record from (a build of the commit to compare against)")
    ap.add_argument("--commit", default=None, help="that commit's id (default: HEAD of the checkout the library lies in)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "beam_dispatch_parent.npz"))
    a = ap.parse_args()
    lib_path = os.path.abspath(a.lib)
    commit = a.commit or subprocess.check_output(["git", "-C", os.path.dirname(lib_path), "rev-parse", "HEAD"], text=True).strip()
    os.environ["PGASR_HIP_LIB"] = lib_path          # read when _lib is imported
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import beam_dispatch_calls as D
    from policy_gradient_asr_amd import _lib
    assert _lib.LIB_PATH == lib_path
    first, second = D.run_all(), D.run_all()
    differ = [n for n in first if first[n] != second[n]]
    if differ or set(first) != set(second):
        sys.exit(f"{len(differ)} of {len(first)} calls differ between two runs, nothing written: {differ[:8]}")
    np.savez_compressed(a.out, commit=np.array(commit), **D.pack(first))
    print(f"{a.out}: {len(first)} calls, {sum(map(len, first.values()))} bytes of output, {os.path.getsize(a.out)} on disk, from {commit[:12]}")


if __name__ == "__main__":
    main()
