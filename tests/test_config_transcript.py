"""The configuration entries of the C ABI (c3d_set_option, c3d_set_model, c3d_set_schedule, c3d_get_stat) on the CPU: the host units run
against the fake HIP layer of tools/sanitize, and tests/harness/config_transcript.cpp writes down what every key does with every value of
its sweep — return code, refusal, the context members that changed.  tests/golden/config_transcript.txt is that text as the commit before
the option and stat tables printed it; tests/test_gpu_config.py holds the shipped library to its codes and refusals on a device."""
import os
import re

import pytest

from tests.util import GOLD, config_transcript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    got = config_transcript()
    if got is None:
        pytest.skip("no host C++ compiler")
    return got


def keys_of(listing, who, kind):
    return [line.split()[2] for line in listing.splitlines() if line.startswith("%s %s " % (who, kind))]


def header_comment_above(declaration):
    """the comment block of include/c3d.h that ends at a declaration"""
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    head = h[:h.index(declaration)]
    return head[head.rindex("/*"):]


def test_the_transcript_is_the_golden_one_byte_for_byte(harness):
    want = open(os.path.join(GOLD, "config_transcript.txt"), newline="").read()
    got = harness[0]
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        diff = [k for k in range(min(len(a), len(b))) if a[k] != b[k]]
        for k in diff[:10]:
            print("line %d\n  now:    %s\n  golden: %s" % (k + 1, a[k], b[k]))
        print("%d lines now, %d golden, %d differ" % (len(a), len(b), len(diff)))
    assert got == want


def test_the_tables_hold_the_keys_the_harness_lists_and_no_others(harness):
    for kind, count in (("option", 39), ("stat", 52)):
        own, table = keys_of(harness[1], "own", kind), keys_of(harness[1], "table", kind)
        assert len(own) == count and len(set(own)) == count
        assert len(table) == len(set(table)), "a key twice in the library's table"
        assert sorted(set(table) - set(own)) == [], "in the library, not in tests/harness/config_transcript.cpp"
        assert sorted(set(own) - set(table)) == [], "in tests/harness/config_transcript.cpp, not in the library"


def test_every_option_is_described_in_the_header(harness):
    doc = header_comment_above("int c3d_set_option(")
    for key in keys_of(harness[1], "table", "option"):
        assert re.search(r"(?<![a-z0-9_])%s(?![a-z0-9_])" % key, doc), key


def test_every_stat_is_named_in_the_header(harness):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    for key in keys_of(harness[1], "table", "stat"):
        assert '"%s"' % key in h, key
