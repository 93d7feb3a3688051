"""A step's kind is named in one place, chromosome3d_amd/csrc/c3d_step_kinds.h: the header pins every name to the number c3d.h and
DevStep document, its predicates hold for the kinds they are defined for and no others, no other source compares a `kind` against a
digit (the exceptions restate the public contract and are listed by file and entry), and the table test hooks are out of the executor.
No GPU."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "chromosome3d_amd", "csrc")
HEADER = os.path.join(SRC, "c3d_step_kinds.h")

# the numbers are ABI (include/c3d.h for the stage kinds, DevStep::kind for all nine)
NUMBERS = {"kMdCouple": 0, "kMdRescale": 1, "kFire": 2, "kFireFirst": 3, "kMdBegin": 4, "kTwoPoint": 5, "kTwoPointFirst": 6,
           "kLbfgs": 8, "kLbfgsFirst": 9}
# every fact the header states, as the set of kinds it holds for
FACTS = {
    "kind_is_md": {0, 1, 4}, "kind_is_fire": {2, 3}, "kind_is_two_point": {5, 6}, "kind_is_lbfgs": {8, 9}, "kind_is_first": {3, 6, 9},
    "kind_reads_sums": {0, 1, 2, 5}, "kind_continues_state": {2, 5}, "kind_stores_state": {2, 3, 5, 6}, "kind_has_no_velocity": {3, 6},
    "stage_is_minimiser": {2, 5, 8},
}
KIND_AGAINST_DIGIT = re.compile(r"kind\s*(==|!=|<=|>=|<|>)\s*\d")
# Where a kind is still compared against digits: file -> entry (the text its definition begins with) -> the lines.  They restate c3d.h's
# contract in the words of the refusal next to them, and the ABI tests read them there.
EXCEPTIONS = {
    "c3d_config.cpp": {
        'extern "C" int c3d_set_schedule(': [
            'if (st[k].kind < 0 || (st[k].kind > 2 && st[k].kind != 5 && st[k].kind != 8) || st[k].nsteps < 0) return fail(C3D_ERR_INVALID, "c3d_set_schedule: bad stage");',
        ],
    },
    "c3d_debug.cpp": {
        'extern "C" int c3d_debug_step_scalars(': ["if (!(kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 5 || kind == 6))"],
        'extern "C" int c3d_debug_row_finish(': ['if (kind < 0 || kind > 6) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish: kind is 0, 1, 2, 3, 4, 5 or 6");'],
        # the refusal check of c3d_debug_step_scalars_f64 and c3d_debug_row_finish_f64
        "bool f64_table_kind(int kind, bool row_finish) {": [
            "return kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 5 || kind == 6 || (row_finish && kind == 4);",
        ],
    },
}


def test_the_header_pins_every_name_to_its_documented_number():
    text = open(HEADER).read()
    enum = text[text.index("enum StepKind : int {"):]
    enum = enum[:enum.index("};")]
    named = {name: int(value) for name, value in re.findall(r"^\s*(k\w+) = (\d+),", enum, re.M)}
    pinned = {name: int(value) for name, value in re.findall(r"^static_assert\((k\w+) == (\d+),", text, re.M)}
    assert named == NUMBERS and pinned == NUMBERS
    # all nine as DevStep::kind documents them, the stage kinds as c3d.h does
    internal = open(os.path.join(SRC, "c3d_internal.h")).read()
    doc = internal[internal.index("int kind;        //"):internal.index("    float dt;")]
    assert sorted(int(d) for d in re.findall(r"(?:: |, |// )(\d) [A-Za-z]", doc)) == sorted(NUMBERS.values())
    public = open(os.path.join(ROOT, "include", "c3d.h")).read()
    doc = public[public.index("int32_t kind;      /*"):public.index("int32_t nsteps;")]
    stage_kinds = sorted(int(d) for d in re.findall(r"(?:/\* |, |\n +)(\d) (?:MD|FIRE|minimise|L-BFGS)", doc))
    assert stage_kinds == [0, 1, 2, 5, 8]
    assert set(stage_kinds) == FACTS["kind_is_md"] - {NUMBERS["kMdBegin"]} | FACTS["stage_is_minimiser"]
    assert '#include "c3d_step_kinds.h"' in internal


def test_every_fact_holds_for_its_kinds_and_no_others():
    """the header as a host compiler sees it: every predicate over kinds 0 .. 9"""
    calls = "\n".join(f'    std::printf("{name}"); for (int k = 0; k < 10; ++k) if (c3d::{name}(k)) std::printf(" %d", k); std::printf("\\n");'
                      for name in FACTS)
    with tempfile.TemporaryDirectory() as tmp:
        main = os.path.join(tmp, "facts.cpp")
        with open(main, "w") as f:
            f.write(f'#include <cstdio>\n#include "{HEADER}"\nint main() {{\n{calls}\n    return 0;\n}}\n')
        exe = os.path.join(tmp, "facts")
        subprocess.run(["g++", "-std=c++17", "-O0", "-D__host__=", "-D__device__=", main, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {line.split()[0]: {int(k) for k in line.split()[1:]} for line in out.splitlines()}
    assert got == FACTS


def test_no_kind_is_compared_against_a_digit():
    for name in sorted(os.listdir(SRC)):
        if name == "c3d_step_kinds.h" or not name.endswith((".h", ".hip", ".inc", ".cpp")):
            continue
        text = open(os.path.join(SRC, name)).read()
        allowed = []
        for entry, lines in EXCEPTIONS.get(name, {}).items():
            assert text.count(entry) == 1, (name, entry)
            body = text[text.index(entry):]
            body = body[:body.index("\n}\n")]
            for line in lines:
                assert line in body, (name, entry, line)          # the exception is still what this list says it is
            allowed += lines
        for line in text.splitlines():
            if KIND_AGAINST_DIGIT.search(line):
                assert line.strip() in allowed, (name, line.strip())
    assert not set(EXCEPTIONS) - set(os.listdir(SRC))


def test_the_table_hooks_are_out_of_the_executor():
    run = open(os.path.join(SRC, "c3d_run.cpp")).read()
    assert 'extern "C" int c3d_debug_' not in run
    assert "is_two_point(int" not in run and "is_lbfgs(int" not in run          # the header's predicates, not a unit's own
    debug = open(os.path.join(SRC, "c3d_debug.cpp")).read()
    for hook in ("c3d_debug_step_scalars", "c3d_debug_row_finish", "c3d_debug_step_scalars_f64", "c3d_debug_row_finish_f64",
                 "c3d_debug_lbfgs_direction", "c3d_debug_lbfgs_move_rows"):
        assert debug.count(f'extern "C" int {hook}(') == 1, hook
    assert 'extern "C" const char* c3d_step_kernel_name(' in run
    config = open(os.path.join(SRC, "c3d_config.cpp")).read()
    assert "c3d::DevFire dev_fire(const c3d_ctx* c) {" in config and "c3d::DevFire dev_fire(const c3d_ctx* c);" in open(os.path.join(SRC, "c3d_ctx.h")).read()
