#!/usr/bin/env python
"""Record tests/golden/ctc_dispatch_parent.npz: a SHA-256 of the status and every output word of each call of
tests/ctc_dispatch_calls.py on ANOTHER commit's library, on the MI355X, in a process of its own:

    timeout -k 10 300 python tools/dev/ctc_dispatch_record.py --lib ../parent/policy_gradient_asr_amd/libpgasr_hip.so --commit <id>

The library is selected with PGASR_HIP_LIB.  --tree DIR imports the Python package of that checkout too (default: this one's), so that
the recording owes nothing to this tree's wrappers.  Every call is made twice; the file is written only if no digest differs between the
two runs, so that it cannot encode run-to-run variation.
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
    ap.add_argument("--tree", default=ROOT, help="the checkout whose policy_gradient_asr_amd package makes the calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ctc_dispatch_parent.npz"))
    a = ap.parse_args()
    lib_path = os.path.abspath(a.lib)
    commit = a.commit or subprocess.check_output(["git", "-C", os.path.dirname(lib_path), "rev-parse", "HEAD"], text=True).strip()
    assert len(commit) == 40
    os.environ["PGASR_HIP_LIB"] = lib_path          # read when _lib is imported
    sys.path[:0] = [os.path.abspath(a.tree), os.path.join(ROOT, "tests")]
    import ctc_dispatch_calls as D
    from policy_gradient_asr_amd import _lib
    assert _lib.LIB_PATH == lib_path and os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.tree) + os.sep)
    first, second = D.run_all(), D.run_all()
    differ = [n for n in first if first[n] != second.get(n)]
    if differ or set(first) != set(second):
        sys.exit(f"{len(differ)} of {len(first)} calls differ between two runs, nothing written: {differ[:8]}")
    np.savez_compressed(a.out, commit=np.array(commit), **D.pack(first))
    print(f"{a.out}: {len(first)} calls, {os.path.getsize(a.out)} bytes on disk, from {commit[:12]}")


if __name__ == "__main__":
    main()
