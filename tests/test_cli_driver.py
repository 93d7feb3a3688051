"""The drop-in boundary as a user meets it: c3d_solve (stand-in for `cns_solve < dgsa.inp`),
c3d_score (spearman_IF_pdb.pl) and the Perl driver with the reference's command line."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import GOLD, golden, load_if, model_pdb, REF_SPEARMAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "chromosome3d_amd", "_lib")
MATRIX = os.path.join(GOLD, "inputs", "chr21_1mb_matrix.txt")
G = golden()


def test_c3d_score_matches_reference_table(built):
    out = subprocess.run([os.path.join(LIBDIR, "c3d_score"), MATRIX, model_pdb("chr21_1mb")], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "SRCC\tPDB" and lines[1].split("\t")[0] == "%.3f" % REF_SPEARMAN["chr21_1mb"]
    bad = subprocess.run([os.path.join(LIBDIR, "c3d_score"), MATRIX, model_pdb("chr13_1mb")], capture_output=True, text=True)
    assert bad.returncode != 0 and "mismatch in size" in bad.stderr


def test_c3d_solve_fails_loudly_without_gpu(built, tmp_path):
    """Error convention of the reference's job.sh (:281-283): non-zero exit + iam.failed."""
    from chromosome3d_amd import lib
    if lib.load().c3d_device_count() > 0:
        pytest.skip("a GPU is visible")
    out = subprocess.run([os.path.join(LIBDIR, "c3d_solve"), "--if", MATRIX, "--out", str(tmp_path), "-m", "2"],
                         capture_output=True, text=True)
    assert out.returncode != 0
    assert (tmp_path / "iam.failed").exists() and not (tmp_path / "iam.running").exists()
    assert "no HIP device" in out.stderr


@pytest.mark.gpu
def test_c3d_solve_cli_end_to_end(built, tmp_path):
    out = subprocess.run([os.path.join(LIBDIR, "c3d_solve"), "--if", MATRIX, "--out", str(tmp_path), "-m", "6"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    cid = "chr21_1mb_matrix"
    assert hashlib.md5(open(tmp_path / "contact.tbl", "rb").read()).hexdigest() == G["chr21_1mb"]["md5_tbl"]
    assert hashlib.md5(open(tmp_path / f"{cid}.dist", "rb").read()).hexdigest() == G["chr21_1mb"]["md5_dist"]
    assert not (tmp_path / "iam.running").exists() and not (tmp_path / "iam.failed").exists()
    pdbs = sorted(tmp_path.glob(f"{cid}_*.pdb"))
    assert len(pdbs) == 6
    # the same restraints through the cns_solve-shaped entry (--tbl) give the same models
    t2 = tmp_path / "tbl_run"
    out2 = subprocess.run([os.path.join(LIBDIR, "c3d_solve"), "--tbl", str(tmp_path / "contact.tbl"), "--n", "37",
                           "--out", str(t2), "--id", cid, "-m", "6"], capture_output=True, text=True)
    assert out2.returncode == 0, out2.stderr
    for p in pdbs:
        a = [l for l in open(p) if l.startswith("ATOM")]
        b = [l for l in open(t2 / p.name) if l.startswith("ATOM")]
        assert a == b
    sc = subprocess.run([os.path.join(LIBDIR, "c3d_score"), MATRIX, str(tmp_path)], capture_output=True, text=True)
    vals = [float(l.split("\t")[0]) for l in sc.stdout.strip().splitlines()[1:]]
    assert len(vals) == 6 and all(-0.95 < v < -0.75 for v in vals)


@pytest.mark.gpu
def test_perl_driver_same_cli_and_outputs(built, tmp_path):
    """chromosome3D.pl's interface: -i (and the -if spelling test.sh uses), -o, -k, -a, -m."""
    if shutil.which("perl") is None:
        pytest.skip("no perl on this box")
    drv = os.path.join(ROOT, "bin", "chromosome3D_amd.pl")
    have_xs = os.path.exists(os.path.join(ROOT, "bindings", "perl", "blib", "auto", "C3D", "C3D.so"))
    # -i through the in-process XS binding (when built), -if through the job.sh / c3d_solve process boundary
    for flag, force_cli in (("-i", "0"), ("-if", "1")):
        od = tmp_path / f"out{flag}"
        env = dict(os.environ, C3D_FORCE_CLI=force_cli) if force_cli == "1" else {k: v for k, v in os.environ.items() if k != "C3D_FORCE_CLI"}
        out = subprocess.run(["perl", drv, flag, MATRIX, "-o", str(od), "-m", "7"], capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("through the C3D XS binding" in out.stdout) == (have_xs and force_cli == "0")
        cid = "chr21_1mb_matrix"
        assert open(od / f"{cid}.fasta").read() == f">{cid}\n" + "M" * 37 + "\n"      # :92-98, one MET per bead
        for f in (f"{cid}.txt", f"{cid}.dist", f"{cid}.rr", "contact.tbl", "job.log", "model_info.log"):
            assert (od / f).exists(), f
        assert open(od / "contact.tbl", "rb").read() == open(os.path.join(GOLD, "chr21_1mb.contact.tbl"), "rb").read()
        models = sorted(od.glob(f"{cid}_model*.pdb"))
        assert [m.name for m in models] == [f"{cid}_model{k}.pdb" for k in range(1, 6)]
        assert len(list(od.glob(f"{cid}_*.pdb"))) == 7
        assert "Restraints : 528 lines in tbl file" in out.stdout and "model1.pdb <=" in out.stdout
        # contact_violation.txt in the reference's row format (:475-483; golden rows from the reference itself)
        import re
        vrows = open(od / "contact_violation.txt").read().splitlines()
        assert len(vrows) == 7 * (2 + 528) and vrows[0].startswith("#NOE violation check;")
        gold_fmt = open(os.path.join(GOLD, "chr21_1mb.contact_violation.txt")).read().splitlines()[2]
        pat = re.compile(r"^  [01]\t-?\d+\.\d\d\t\d+\.\d\d # assign45  resid +\d+ and name ca   resid +\d+ and name ca  \d+\.\d0 0\.00 0\.00$")
        assert pat.match(gold_fmt), gold_fmt
        assert all(pat.match(r) for r in vrows[2:530])
        # the final files are shaped as assess_dgsa leaves them (:813-820): ATOM rows, an empty line, CONECT rows, END;
        # the REMARK rows went to model_info.log behind the file's name (reference :870-873)
        for m in list(od.glob(f"{cid}_*.pdb")):
            rows = open(m).read().split("\n")
            assert all(r.startswith("ATOM") for r in rows[:37]) and rows[37] == "" and rows[38] == "CONECT    1    2"
            assert rows[-2] == "END" and rows[-1] == "" and len(rows) == 37 + 1 + 36 + 2
        log = open(od / "model_info.log").read()
        noe = {m_.group(1): int(float(m_.group(2))) for m_ in re.finditer(r"\./(\S+?\.pdb)REMARK FILENAME.*?REMARK noe = ([-0-9.e+]+)", log, re.S)}
        assert len(noe) == 7
        # ranking = ascending int(REMARK noe) (:796-802, :822-828)
        picked = [l.split("<=")[1].strip().lstrip("./") for l in out.stdout.splitlines() if re.match(r"model\d\.pdb <=", l)]
        assert len(picked) == 5
        e = [noe[pk] for pk in picked]
        assert e == sorted(e) and max(e) <= min(v for k, v in noe.items() if k not in picked)
        # satisfaction table rows "count/528  sumdev  name" agree with the library's assessment
        from chromosome3d_amd import pipeline
        rows = pipeline.read_tbl(str(od / "contact.tbl"))
        tab = [l.split() for l in out.stdout.splitlines() if "/528" in l]
        assert len(tab) == 7
        name_to_row = {t[2]: t for t in tab}
        x = pipeline.read_pdb_ca(str(models[0]))
        first = [l for l in out.stdout.splitlines() if l.startswith("model1.pdb <=")][0].split("<=")[1].strip()
        sat, dev = pipeline.assess(x, rows)
        t = name_to_row[os.path.basename(first)[:-4]]
        assert t[0] == f"{sat}/528" and t[1] == "%.2f" % dev
    # bad usage -> non-zero exit like the reference's print_usage / confess
    assert subprocess.run(["perl", drv, "-o", str(tmp_path / "x")], capture_output=True).returncode != 0
    assert subprocess.run(["perl", drv, "-i", "/nonexistent.txt", "-o", str(tmp_path / "x")], capture_output=True).returncode != 0


@pytest.mark.gpu
def test_batch_script_runs_every_matrix(built, tmp_path):
    """test.sh twin: one job per *_matrix.txt, logs + ranked models per chromosome."""
    if shutil.which("perl") is None:
        pytest.skip("no perl on this box")
    ind = tmp_path / "in"
    ind.mkdir()
    for cid in ("chr21_1mb", "chr22_1mb"):
        shutil.copy(os.path.join(GOLD, "inputs", f"{cid}_matrix.txt"), ind)
    out = subprocess.run(["bash", os.path.join(ROOT, "bin", "run_all_amd.sh"), str(ind), str(tmp_path / "out"), "1", "-m", "6"],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    for cid in ("chr21_1mb", "chr22_1mb"):
        assert (tmp_path / "out" / f"{cid}.log").exists()
        assert len(list((tmp_path / "out" / cid).glob(f"{cid}_matrix_model*.pdb"))) == 5


@pytest.mark.gpu
def test_accepted_twins_are_written_deduplicated_and_ranked_as_the_reference_does(built, tmp_path):
    """The reference's deck writes <ID>a_<k>.pdb beside <ID>_<k>.pdb for structures CNS accepts; job.sh takes either as success
    (chromosome3D.pl:266-277) and assess_dgsa deletes the trial twin of every accepted file before it ranks (:790-795).  `c3d_solve
    --accepted` / the driver's `-accepted` write the twins (every model: CNS's acceptance thresholds are defined on covalent geometry a
    bead model does not have); through both binding routes the trial twins are gone afterwards, the accepted files were ranked, and the
    five models are byte for byte those of a run without the option."""
    if shutil.which("perl") is None:
        pytest.skip("no perl on this box")
    drv = os.path.join(ROOT, "bin", "chromosome3D_amd.pl")
    cid = "chr21_1mb_matrix"
    plain = tmp_path / "plain"
    out = subprocess.run(["perl", drv, "-i", MATRIX, "-o", str(plain), "-m", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for force_cli in ("0", "1"):
        od = tmp_path / f"acc{force_cli}"
        env = dict(os.environ, C3D_FORCE_CLI="1") if force_cli == "1" else {k: v for k, v in os.environ.items() if k != "C3D_FORCE_CLI"}
        out = subprocess.run(["perl", drv, "-i", MATRIX, "-o", str(od), "-m", "7", "-accepted"], capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.count(f"deleting {cid}_") == 7 and f"because {cid}a_7.pdb exists!" in out.stdout
        left = sorted(p.name for p in od.glob("*.pdb"))
        assert sum(n.startswith(f"{cid}a_") for n in left) == 2 and sum("_model" in n for n in left) == 5 and len(left) == 7, left
        picked = [l.split("<=")[1].strip() for l in out.stdout.splitlines() if l.startswith("model") and "<=" in l]
        assert len(picked) == 5 and all(f"{cid}a_" in q for q in picked), picked
        for k in range(1, 6):
            assert open(od / f"{cid}_model{k}.pdb").read() == open(plain / f"{cid}_model{k}.pdb").read(), k
    # the executable alone: both files of every model, same bytes but for the name rows
    od = tmp_path / "solve"
    out = subprocess.run([os.path.join(LIBDIR, "c3d_solve"), "--if", MATRIX, "--out", str(od), "-m", "3", "--accepted"], capture_output=True, text=True)
    assert out.returncode == 0 and "trial and accepted structures written." in out.stdout, out.stdout + out.stderr
    for k in (1, 2, 3):
        a = [l for l in open(od / f"{cid}_{k}.pdb") if not l.startswith("REMARK FILENAME")]
        b = [l for l in open(od / f"{cid}a_{k}.pdb") if not l.startswith("REMARK FILENAME")]
        assert a == b and len(a) > 37


def test_perl_driver_seq_option_cannot_reach_a_shell(built, tmp_path):
    """-seq <fasta> names residues (reference :93-98).  A hostile FASTA (stop codon '*', ';', '$( )', backticks) is refused before
    anything runs; a clean one travels to c3d_solve as `--seq '@<ID>.fasta'` — the file the driver wrote — and every string on the
    job.sh line is single-quoted.  No GPU needed: the solver is a stand-in script that records its arguments."""
    if shutil.which("perl") is None:
        pytest.skip("no perl here")
    drv = os.path.join(ROOT, "bin", "chromosome3D_amd.pl")
    canary = tmp_path / "canary"
    for k, text in enumerate((">x\nMKV*\n", ">x\nMKV;touch " + str(canary) + "\n", ">x\nM$(touch " + str(canary) + ")K\n", ">x\nM`touch " + str(canary) + "`K\n")):
        fa = tmp_path / f"bad{k}.fasta"
        fa.write_text(text)
        out = subprocess.run(["perl", drv, "-i", MATRIX, "-o", str(tmp_path / f"bad{k}"), "-m", "2", "-seq", str(fa)],
                             capture_output=True, text=True, env=dict(os.environ, C3D_FORCE_CLI="1"))
        assert out.returncode != 0 and "residue codes must be letters" in out.stderr, out.stderr
        assert not canary.exists() and not (tmp_path / f"bad{k}" / "job.sh").exists()
    fake = tmp_path / "fake_solve.sh"
    fake.write_text("#!/bin/bash\nprintf '%s\\n' \"$@\" > args.txt\nexit 3\n")
    fake.chmod(0o755)
    fa = tmp_path / "ok.fasta"
    fa.write_text(">x\nrsedw\nQC\n")
    od = tmp_path / "ok"
    out = subprocess.run(["perl", drv, "-i", MATRIX, "-o", str(od), "-m", "2", "-seq", str(fa)], capture_output=True, text=True,
                         env=dict(os.environ, C3D_FORCE_CLI="1", C3D_SOLVE=str(fake)))
    assert out.returncode != 0                                      # the stand-in writes no models: the driver must say so
    cid = "chr21_1mb_matrix"
    assert open(od / f"{cid}.fasta").read() == f">{cid}\nRSEDWQC" + "M" * 30 + "\n"
    args = open(od / "args.txt").read().split("\n")
    assert args[args.index("--seq") + 1] == f"@{cid}.fasta" and args[args.index("--id") + 1] == cid
    line = [l for l in open(od / "job.sh") if "--seq" in l][0]
    assert f"--seq '@{cid}.fasta'" in line and f"--id '{cid}'" in line and "RSEDWQC" not in line


def test_perl_driver_fails_loudly_without_gpu(built, tmp_path):
    """Error convention of the reference (:281-288): iam.failed + die, through both binding routes."""
    from chromosome3d_amd import lib
    if lib.load().c3d_device_count() > 0:
        pytest.skip("a GPU is visible")
    if shutil.which("perl") is None:
        pytest.skip("no perl here")
    drv = os.path.join(ROOT, "bin", "chromosome3D_amd.pl")
    for force_cli in ("0", "1"):
        od = tmp_path / f"o{force_cli}"
        env = dict(os.environ)
        env.pop("C3D_FORCE_CLI", None)
        if force_cli == "1":
            env["C3D_FORCE_CLI"] = "1"
        out = subprocess.run(["perl", drv, "-i", MATRIX, "-o", str(od), "-m", "3"], capture_output=True, text=True, env=env)
        assert out.returncode != 0
        assert (od / "iam.failed").exists()
        assert "no HIP device" in (out.stderr + out.stdout + open(od / "job.log").read() if (od / "job.log").exists() else out.stderr + out.stdout)
        assert not list(od.glob("*_model*.pdb"))


@pytest.mark.gpu
def test_batch_executor_lanes_do_not_change_results(built, tmp_path):
    """c3d_batch (test.sh:4-12 in one process): two matrices, once with one and once with two host lanes per GPU — same ranked
    models byte for byte, the reference's per-chromosome files present."""
    exe = os.path.join(LIBDIR, "c3d_batch")
    ind = os.path.join(GOLD, "inputs")
    outs = []
    for lanes in (1, 2):
        od = tmp_path / f"b{lanes}"
        p = subprocess.run([exe, os.path.join(ind, "chr21_1mb_matrix.txt"), os.path.join(ind, "chr22_1mb_matrix.txt"), "--out", str(od), "--lanes", str(lanes),
                            "-m", "6"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "2 matrices x 6 models" in p.stdout and "0 failed" in p.stdout
        outs.append(od)
    for chrom in ("chr21_1mb", "chr22_1mb"):
        cid = chrom + "_matrix"
        for f in (f"{cid}.dist", f"{cid}.rr", "contact.tbl", f"{cid}.fasta", "model_info.log"):
            assert (outs[0] / chrom / f).exists(), f
        for k in range(1, 6):
            a = open(outs[0] / chrom / f"{cid}_model{k}.pdb").read()
            assert a == open(outs[1] / chrom / f"{cid}_model{k}.pdb").read()
            assert a.count("ATOM") == (37 if chrom == "chr21_1mb" else 35) and a.rstrip().endswith("END")
    # --violations: contact_violation.txt as the reference leaves it (:475-483: 2 + R rows per model, violated rows first), and the
    # satisfaction table of the log — device numbers without the option, the violation writer's with it — does not change
    od = tmp_path / "bv"
    p = subprocess.run([exe, os.path.join(ind, "chr21_1mb_matrix.txt"), "--out", str(od), "--lanes", "1", "-m", "6", "--violations"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    v = open(od / "chr21_1mb" / "contact_violation.txt").read().splitlines()
    assert len(v) == 6 * (2 + 528) and v[0].startswith("#NOE violation check; ./chr21_1mb_matrix_") and v[0].endswith(" against contact.tbl")
    flags = [r[:3] for r in v[2:530]]
    assert flags == sorted(flags, reverse=True) and set(flags) <= {"  1", "  0"}
    table = lambda d: [l for l in open(d / "chr21_1mb.log").read().splitlines() if "/528" in l]
    assert len(table(od)) == 6 and table(od) == table(outs[0])


@pytest.mark.gpu
def test_batch_executor_per_device_lists_and_threads_rehearsed_on_one_gpu(built, tmp_path):
    """c3d_batch --devices N on an N-GPU node (csrc/c3d_batch_main.cpp: LPT over the devices, `lanes` host threads and contexts per
    device) had never executed with N > 1: `--map-devices-to 0` runs that code on this box — four logical devices, two lanes each, all on
    physical device 0 — and the models equal those of `--devices 1` byte for byte; every logical device got work.  A device exception
    would now arrive here in the runtime's own words (the CLI sets HSA_DISABLE_COREDUMP_ON_EXCEPTION: round 5's one failure of this
    start came back as rc -13 out of the runtime's core-dump helper, its cause unnamed)."""
    import re
    exe = os.path.join(LIBDIR, "c3d_batch")
    ind = os.path.join(GOLD, "inputs")
    mats = [os.path.join(ind, f"{c}_matrix.txt") for c in ("chr21_1mb", "chr22_1mb")]
    from tests.util import write_if_text
    for c in ("chr20_1mb", "chr13_1mb", "chr19_500kb", "chr21_500kb"):          # packed fixtures -> the reference's text format
        pth = tmp_path / f"{c}_matrix.txt"
        write_if_text(load_if(c), pth)
        mats.append(str(pth))
    runs = {}
    # "eight": the production shape of an 8-GPU node — 8 devices x 3 lanes = 24 contexts of one process — on this box's one device
    for tag, extra in (("one", ["--devices", "1", "--lanes", "1", "--pair", "0"]), ("four", ["--devices", "4", "--lanes", "2", "--map-devices-to", "0"]),
                       ("paired", ["--devices", "1", "--lanes", "3"]), ("eight", ["--devices", "8", "--lanes", "3", "--map-devices-to", "0"])):
        od = tmp_path / tag
        p = subprocess.run([exe] + mats + ["--out", str(od), "-m", "6"] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "6 matrices x 6 models" in p.stdout and "0 failed" in p.stdout
        runs[tag] = (od, p.stdout)
    assert "on 4 GPU(s), 2 lane(s) each" in runs["four"][1] and "on 8 GPU(s), 3 lane(s) each" in runs["eight"][1]
    assert sorted(set(re.findall(r"GPU (\d)(?: XCDs \d-\d)?  \[phases", runs["four"][1]))) == ["0", "1", "2", "3"]      # every logical device took jobs
    for chrom in ("chr21_1mb", "chr22_1mb", "chr20_1mb", "chr13_1mb", "chr19_500kb", "chr21_500kb"):
        cid = chrom + "_matrix"
        for k in range(1, 6):
            assert open(runs["one"][0] / chrom / f"{cid}_model{k}.pdb").read() == open(runs["four"][0] / chrom / f"{cid}_model{k}.pdb").read(), (chrom, k)
            assert open(runs["one"][0] / chrom / f"{cid}_model{k}.pdb").read() == open(runs["paired"][0] / chrom / f"{cid}_model{k}.pdb").read(), (chrom, k)
            assert open(runs["one"][0] / chrom / f"{cid}_model{k}.pdb").read() == open(runs["eight"][0] / chrom / f"{cid}_model{k}.pdb").read(), (chrom, k)
    # (round 5 ran the eight-context start seven times here to see whether its device exception came back; a pass by not reproducing a
    #  race is no evidence.  Round 6 removed what could race — c3d_create loads every code object a default job needs before it returns,
    #  no helper thread touches the runtime, loads and launches exclude one another: csrc/c3d_gate.cpp "code objects" — and checks THAT on
    #  the CPU under ThreadSanitizer against a fake HIP layer, tests/test_abi_host.py::test_executor_and_loader_under_thread_sanitizer;
    #  the start above runs once, like any other test.)
    # --pair 1 (default), three lanes: the small chromosomes annealed on halves of the device, --pair 0: nobody did
    assert " XCDs " in runs["paired"][1] and " XCDs " not in runs["one"][1]
    bad = subprocess.run([exe] + mats[:1] + ["--out", str(tmp_path / "x"), "--map-devices-to", "7"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--map-devices-to 7" in bad.stderr
