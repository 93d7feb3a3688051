"""The shipped libc3d.so, on a device, against tests/golden/config_transcript.txt: the sweep of every option key over every value and of
every stat key that tests/harness/config_transcript.cpp makes on the CPU — a fresh context per key, as created (state A) and with targets
from a 40 x 40 matrix and 4 replicas (state B) — repeated through ctypes.  Every call must end with the return code and the refusal the
golden file holds for it: the hipcc-built library and the g++-built harness are the same code.  What a call changes inside the context is
not visible through the ABI and is not compared; no step is launched, every call either stores a value or is refused on the host."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.util import GOLD, transcript_calls

pytestmark = pytest.mark.gpu
BEADS, REPLICAS = 40, 4


def golden_blocks(state):
    """[(what, [(call, return code, refusal)])]: the golden file's contexts in `state` that hold option and stat calls only"""
    blocks = {}
    for ctx, st, what, call, rc, refusal, _ in transcript_calls(open(os.path.join(GOLD, "config_transcript.txt")).read()):
        if st == state and not what.startswith(("model", "schedule", "a kind-8 stage", "precision 64")):
            blocks.setdefault((ctx, what), []).append((call, rc, refusal))
    out = []
    for (_, what), lines in sorted(blocks.items()):
        names = [c[0] for c in lines]
        if "(pair targets planted)" in names:                      # the first context of a state shows its set-up: not part of the sweep
            lines = lines[names.index("(pair targets planted)") + 1:]
        out.append((what, lines))
    return out


def fresh_context(L, lib, state):
    h = C.c_void_p()
    lib.check(L.c3d_create(0, C.byref(h)))
    if state == "B":
        i, j = np.indices((BEADS, BEADS))
        IF = np.ascontiguousarray(100.0 / (1 + np.abs(i - j)))
        lib.check(L.c3d_set_if_matrix(h, lib.dptr(IF), BEADS, 0.5, 11.0))
        lib.check(L.c3d_set_option(h, b"cluster", 0.0))
        lib.check(L.c3d_set_option(h, b"resident", 0.0))
        lib.check(L.c3d_init_replicas(h, REPLICAS, 82364, 0))
    return h


def replay(L, h, call):
    """one call of the transcript on the context h -> (return code, c3d_last_error())"""
    words = call.split()
    v = C.c_double()
    ctx = None if call.endswith("(null context)") else h
    if words[0] == "set_option":
        rc = L.c3d_set_option(ctx, None if words[1] == "(null" else words[1].encode(), float(words[2] if words[1] != "(null" else words[3]))
    else:
        assert words[0] == "get_stat", call
        rc = L.c3d_get_stat(ctx, None if words[1] == "(null" else words[1].encode(), None if "(null value)" in call else C.byref(v))
    return rc, L.c3d_last_error().decode() if rc else ""


@pytest.mark.parametrize("state", ["A", "B"])
def test_every_call_ends_as_the_golden_transcript_says(built, state):
    from chromosome3d_amd import lib
    L = lib.load()
    blocks = golden_blocks(state)
    assert sum(what.startswith("option ") for what, _ in blocks) == 39 and any(what == "stats" for what, _ in blocks)
    wrong, calls = [], 0
    for what, lines in blocks:
        h = fresh_context(L, lib, state)
        try:
            for call, rc, refusal in lines:
                got = replay(L, h, call)
                calls += 1
                if got != (rc, refusal):
                    wrong.append((what, call, got, (rc, refusal)))
        finally:
            L.c3d_destroy(h)
    for w in wrong[:20]:
        print("%s | %s: %r, golden %r" % w)
    assert calls >= 39 * 33 + 52 and not wrong, "%d of %d calls differ from the golden transcript" % (len(wrong), calls)
