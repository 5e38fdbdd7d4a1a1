#!/usr/bin/env python
"""Record tests/golden/ctc_status_grid.json: the status of every call of tests/ctc_status_grid.py, and what the workspace-size
queries return, on ANOTHER commit's library.

    git worktree add ../parent <commit> && make -C ../parent/policy_gradient_asr_amd/csrc
    python tools/dev/ctc_status_record.py --lib ../parent/policy_gradient_asr_amd/libpgasr_hip.so

Needs no GPU: no call of the grid reaches HIP.  The commit id written into the file is --commit, or that of the checkout the library
lies in.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the library to record from (a build of the commit to compare against)")
    ap.add_argument("--commit", default=None, help="that commit's id (default: HEAD of the checkout the library lies in)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ctc_status_grid.json"))
    a = ap.parse_args()
    lib_path = os.path.abspath(a.lib)
    commit = a.commit or subprocess.check_output(["git", "-C", os.path.dirname(lib_path), "rev-parse", "HEAD"], text=True).strip()
    assert len(commit) == 40
    os.environ["PGASR_HIP_LIB"] = lib_path          # read when _lib is imported
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import ctc_status_grid as G
    from policy_gradient_asr_amd import _lib
    assert _lib.LIB_PATH == lib_path
    statuses, sizes = G.replay(_lib.load())
    rows = lambda d: ",\n".join('  "%s": %s' % (e, json.dumps(d[e], separators=(",", ":"))) for e in d)      # noqa: E731
    with open(a.out, "w") as f:
        f.write('{"commit": "%s",\n "statuses": {\n%s\n },\n "sizes": {\n%s\n }}\n' % (commit, rows(statuses), rows(sizes)))
    print(f"{a.out}: {sum(len(v) for v in statuses.values())} calls of {len(statuses)} entries and "
          f"{sum(len(v) for v in sizes.values())} size queries on {commit[:12]}")


if __name__ == "__main__":
    main()
