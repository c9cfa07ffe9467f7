"""The generated main-loop statements (constriction_amd/csrc/*.inc) must be exactly what their generators emit: the generators keep
the s_waitcnt book, a hand edit of an .inc would not.  scripts/loops.py holds the manifest (generator, variant knobs, files) and
is the one way to run a generator; nothing here may write into the checked-in tree (constriction_amd/build.py goes by mtime)."""
import importlib.util
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "constriction_amd" / "csrc"


def _load(name):
    sys.path.insert(0, str(ROOT / "scripts"))
    spec = importlib.util.spec_from_file_location(name, ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


loops = _load("loops")


def _mtimes(directory):
    return {p.name: p.stat().st_mtime_ns for p in sorted(Path(directory).glob("*.inc"))}


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """every manifest entry generated once, through the driver, into a directory of its own"""
    out = tmp_path_factory.mktemp("generated")
    before = _mtimes(CSRC)
    assert loops.main(["--out", str(out)]) == 0
    assert _mtimes(CSRC) == before
    return out


@pytest.mark.parametrize("name", loops.FILES)
def test_loop_is_in_sync(generated, name):
    assert (generated / name).read_bytes() == (CSRC / name).read_bytes()


def test_manifest_lists_every_statement_and_nothing_else(generated):
    statements = {p.name for p in CSRC.glob("*.inc") if "asm volatile(" in p.read_text()}
    assert statements == set(loops.FILES)
    assert len(loops.FILES) >= 77
    assert {p.name for p in generated.iterdir()} == set(loops.FILES)


def test_the_check_writes_nothing_into_the_tree():
    before = _mtimes(CSRC)
    assert len(before) >= 77
    assert loops.main(["--check"]) == 0
    assert _mtimes(CSRC) == before


def test_ambient_knobs_change_nothing():
    """variant knobs are no environment variables any more, and experiment knobs do not reach a --check"""
    env = dict(os.environ, GEN_PT_SUB="2", GEN_RANGE_N8="1", GEN_NO_LGKM="1", GEN_ALIGN="0")
    res = subprocess.run([sys.executable, str(ROOT / "scripts" / "loops.py"), "--check"], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(loops.FILES)} files, 0 stale" in res.stdout


def test_experiment_loops_never_go_into_the_tree(monkeypatch):
    monkeypatch.setenv("GEN_NO_LGKM", "1")
    with pytest.raises(SystemExit):
        loops.main(["--experiment"])
    with pytest.raises(SystemExit):
        loops.main(["--experiment", "--out", str(CSRC)])


def test_a_stale_file_is_found(tmp_path, capsys):
    for name in loops.FILES:
        shutil.copy(CSRC / name, tmp_path / name)
    victim = tmp_path / "cst_range_decode_loop_b16_sub_n8.inc"
    text = victim.read_bytes()
    victim.write_bytes(text[:1000] + bytes([text[1000] ^ 1]) + text[1001:])
    capsys.readouterr()
    assert loops.main(["--check", "--out", str(tmp_path)]) == 1
    reported = [ln.split()[-1] for ln in capsys.readouterr().out.splitlines() if ln.startswith("stale: ")]
    assert reported == [str(victim)]


def test_writing_is_idempotent(generated):
    before = _mtimes(generated)
    assert len(before) == len(loops.FILES)
    assert loops.main(["--out", str(generated)]) == 0
    assert _mtimes(generated) == before


def test_an_undeclared_knob_is_an_error():
    with pytest.raises(TypeError, match="declares no variant knob"):
        loops.run("gen_pt_decode_loop", {"sub": 1, "packed": True}, ("cst_pt_decode_loop_sub.inc",))
    with pytest.raises(TypeError, match="declares no variant knob"):          # ... a generator without knobs included
        loops.run("gen_decode_loop_dq", {"n8": True}, ("cst_decode_loop_dq.inc",))


def test_a_run_must_make_exactly_its_files():
    with pytest.raises(RuntimeError, match="the manifest lists"):
        loops.run("gen_decode_loop", {}, ("cst_decode_loop.inc",))


def test_wait_bookkeeping_rejects_unreachable_counts():
    """asmgen refuses a wait whose operand would exceed what the hardware counter can express."""
    asmgen = _load("asmgen")
    a = asmgen.Asm()
    a.ds("ds_read_b32 v0, v1", "first")
    for k in range(16):
        a.ds(f"ds_read_b32 v{2 + k}, v1", "later")
    try:
        a.wait_lds("first")
    except AssertionError:
        return
    raise AssertionError("lgkmcnt operand > 15 must be rejected")


def test_every_loop_head_is_pinned_to_a_cache_line():
    """code placement is worth +-10 % on these loops (profiles/r04_placement.txt): every generated statement carries
    `.p2align 6` directly in front of its loop head, so that an edit upstream of a loop cannot move it (asmgen.py)"""
    incs = sorted((ROOT / "constriction_amd" / "csrc").glob("*.inc"))
    statements = [p for p in incs if "asm volatile(" in p.read_text()]
    assert len(statements) >= 40
    for p in statements:
        lines = [ln.split("//")[0].strip() for ln in p.read_text().splitlines()]
        heads = [i for i, ln in enumerate(lines) if ln == '"1:\\n"']
        assert len(heads) == 1, p.name
        assert lines[heads[0] - 1] == '".p2align 6\\n\\t"', p.name


def test_every_statement_declares_scc_clobbered():
    """the generated statements count tiles and compare on the scalar side (s_sub_u32 / s_cmp_* / s_add_u32 ...: all write SCC).  Until
    round 5 none declared it, and one harmless edit made the compiler keep a flag in SCC ACROSS a statement"""
    incs = sorted((ROOT / "constriction_amd" / "csrc").glob("*.inc"))
    statements = [p for p in incs if "asm volatile(" in p.read_text()]
    assert len(statements) >= 40
    for p in statements:
        text = p.read_text()
        clobbers = text[text.rindex("    : "):]
        assert '"scc"' in clobbers and '"vcc"' in clobbers and '"memory"' in clobbers, p.name
