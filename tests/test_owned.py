"""Who frees what in the host code (smallk_amd/csrc/owned.h): a handle's device blocks, pinned blocks, events and streams are
created through its Owned member and released by it alone; a function's scratch lives in a Scratch.  Hygiene, on the CPU:
solver.cpp and matrix.cpp release nothing by hand, state.h keeps no field whose only use is to remember what to free, and
no kernel file sees the header."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallk_amd", "csrc")
# the host files behind the two handles: the solver's (solver.cpp and what was cut out of it) and the matrix's
HOST = ("solver.cpp", "progress.cpp", "attach.cpp", "factors.cpp", "guard.cpp", "timing.cpp", "standalone.cpp", "matrix.cpp")
FREES = re.compile(r"dev_free|hipHostFree|hipEventDestroy|hipStreamDestroy|hipFree")


def lines(name):
    return list(enumerate(open(os.path.join(CSRC, name), errors="replace"), 1))


def test_handles_release_through_their_owner_only():
    stray = ["%s:%d" % (f, i) for f in HOST + ("state.h", "solver_internal.h") for i, l in lines(f) if FREES.search(l)]
    assert not stray, stray
    # ... and create nothing behind the owner's back: events, streams and pinned memory only inside owned.h
    makes = re.compile(r"hipEventCreate|hipStreamCreate|hipHostMalloc|hipMalloc")
    stray = ["%s:%d" % (f, i) for f in HOST + ("state.h", "solver_internal.h") for i, l in lines(f) if makes.search(l)]
    assert not stray, stray
    # a device allocation outside the owner goes into a Scratch (dev_malloc by bytes through put())
    raw = [(f, i, l) for f in HOST for i, l in lines(f) if "dev_malloc(" in l or re.search(r"(?<![\w.])dev_alloc\(", l)]
    assert all(".put()" in l for _, _, l in raw), [(f, i) for f, i, l in raw if ".put()" not in l]
    # both handles have one owner; the fields that only remembered what to free are gone
    state = open(os.path.join(CSRC, "state.h")).read()
    assert len(re.findall(r"\bsmk::Owned own;", state)) == 2
    assert not re.search(r"\b(Wt_own|Gh_own|scal_own)\b", state + "".join(open(os.path.join(CSRC, f)).read() for f in HOST))
    # the owner is the one place that frees all four kinds
    owned = open(os.path.join(CSRC, "owned.h")).read()
    for call in ("dev_free", "hipHostFree", "hipEventDestroy", "hipStreamDestroy"):
        assert call in owned, call


def test_owned_h_stays_out_of_the_kernel_files():
    users = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and '"owned.h"' in open(p, errors="replace").read())
    assert not [u for u in users if u.endswith(".hip") or u == "common.h"], users
    assert {"state.h"} <= set(users) <= {"state.h", "solver.cpp", "matrix.cpp", "preprocess.cpp"}, users
