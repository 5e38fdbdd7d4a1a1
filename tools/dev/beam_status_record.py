#!/usr/bin/env python
"""Record tests/golden/beam_status_grid.json: the status of every call of tests/beam_status_grid.py on ANOTHER commit's library.

    git worktree add ../parent <commit> && make -C ../parent/policy_gradient_asr_amd/csrc
    python tools/dev/beam_status_record.py --lib ../parent/policy_gradient_asr_amd/libpgasr_hip.so

Needs no GPU: no call of the grid reaches HIP.  The commit id written into the file is that of the checkout the library lies in.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "beam_status_grid.json"))
    a = ap.parse_args()
    lib_path = os.path.abspath(a.lib)
    commit = subprocess.check_output(["git", "-C", os.path.dirname(lib_path), "rev-parse", "HEAD"], text=True).strip()
    os.environ["PGASR_HIP_LIB"] = lib_path          # read when _lib is imported
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import beam_status_grid as G
    from policy_gradient_asr_amd import _lib
    assert _lib.LIB_PATH == lib_path
    grid = G.replay(_lib.load())
    with open(a.out, "w") as f:
        f.write('{"commit": "%s",\n "statuses": {\n' % commit)
        f.write(",\n".join('  "%s": %s' % (e, json.dumps(grid[e], separators=(",", ":"))) for e in grid))
        f.write("\n }}\n")
    print(f"{a.out}: {sum(len(v) for v in grid.values())} calls of {len(grid)} entries on {commit[:12]}")


if __name__ == "__main__":
    main()
