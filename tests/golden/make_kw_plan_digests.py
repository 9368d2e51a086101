"""Writes tests/golden/kw_plan_digests.json: the plan digests (typesense_amd/csrc/kw_plan_digest.h) of every batch of tests/kw_plan_digest_common.py.

The fixture pins the planner across a restructuring, so it is recorded from the commit BEFORE that restructuring, never from the tree under test:
check the parent commit out into a scratch directory, add only the digest hook to it (kw_plan_digest.h, the option, the two counters and the call in
kw_batch_on_lane's staging section), build its emulator library (tests/hipemu/build_emu.sh) and pass that library here.
Run: python tests/golden/make_kw_plan_digests.py <path to the parent's libtsgpu_emu.so>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kw_plan_digest_common as C  # noqa: E402


class Anything:                      # stands in for the fixture while it is being recorded: equal to every digest
    def __eq__(self, other): return True
    def __getitem__(self, key): return self


C.golden = Anything
JOBS = [("mixed", None), ("wildcard", None), ("planners", None), ("cap", None)] + [("grid", n) for n in C.BATCH_SIZES]


def record(job):                     # one world per job: the jobs run side by side (the emulator takes minutes over the 2 100-query batches)
    kind, n = job
    if kind == "cap":
        return C.body_block_cap(sys.argv[1])
    w = C.World(sys.argv[1])
    if kind == "mixed": C.body_mixed_batch(w)
    elif kind == "wildcard": C.body_wildcard(w)
    elif kind == "planners": C.body_both_planners(w, True)
    else: C.body_option_grid(w, n)
    w.close()
    return w.seen


if __name__ == "__main__":
    from concurrent.futures import ProcessPoolExecutor
    seen = {}
    with ProcessPoolExecutor(len(JOBS)) as pool:
        for part in pool.map(record, JOBS):
            seen.update(part)
    with open(C.GOLDEN, "w") as f:
        json.dump(dict(sorted(seen.items())), f, indent=0)
        f.write("\n")
    print("%d cases -> %s" % (len(seen), C.GOLDEN))
