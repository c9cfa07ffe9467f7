#!/usr/bin/env python3
"""The manifest of the generated main-loop statements (constriction_amd/csrc/*.inc) and the one way to make them.

LOOPS lists every generator run: the generator, its variant knobs, and exactly the files that run produces.  The files
are checked in; the generators keep the s_waitcnt book, so nobody edits an .inc by hand.

    python scripts/loops.py                 regenerate constriction_amd/csrc (writes only what differs, prints what changed)
    python scripts/loops.py --check         write nothing; list the stale files, exit 1 if there are any
    python scripts/loops.py --out DIR       generate into DIR instead
    python scripts/loops.py --only GEN      only the runs of one generator (gen_pt_decode_loop)

Two classes of knob.  VARIANT knobs select a checked-in file; they stand in LOOPS and reach the generator as parameters
(asmgen.knobs).  EXPERIMENT knobs (GEN_NO_LGKM, GEN_ALIGN, GEN_NSETS ...: results wrong on purpose, or placement studies)
are environment variables that only `--experiment --out DIR` lets through: every other run generates with all GEN_*
variables removed, and an experiment loop never goes into constriction_amd/csrc.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
from pathlib import Path

SCRIPTS = Path(__file__).resolve().parent
CSRC = SCRIPTS.parent / "constriction_amd" / "csrc"


def _names(stem, *suffixes):
    return tuple(f"{stem}{s}.inc" for s in suffixes)


# (generator, variant knobs, files)
LOOPS = (
    ("gen_encode_loop", {}, _names("cst_encode_loop", "", "_1buf", "_sm")),
    ("gen_decode_loop", {}, _names("cst_decode_loop", "", "_sm")),
    ("gen_decode_loop_small", {}, ("cst_decode_loop_small.inc",)),
    ("gen_decode_loop_small", {"n8": 8}, ("cst_decode_loop_small_n8.inc",)),
    ("gen_decode_loop_small", {"n8": 16}, ("cst_decode_loop_small_n16.inc",)),
    ("gen_decode_loop_n8", {}, ("cst_decode_loop_n8.inc",)),
    ("gen_decode_loop_n8", {"n16": True}, ("cst_decode_loop_n16.inc",)),
    ("gen_decode_loop_dq", {}, ("cst_decode_loop_dq.inc",)),
    ("gen_decode_loop_b16", {}, _names("cst_decode_loop_b16", "", "_sm")),
    ("gen_decode_loop_b16", {"narrow": 1}, ("cst_decode_loop_b16_n8.inc",)),
    ("gen_decode_loop_b16", {"narrow": 2}, ("cst_decode_loop_b16_n16.inc",)),
    ("gen_decode_loop_b16", {"small": True, "narrow": 1}, ("cst_decode_loop_b16_s8.inc",)),
    ("gen_decode_loop_b16", {"small": True, "narrow": 2}, ("cst_decode_loop_b16_s16.inc",)),
    ("gen_decode_loop_b16", {"small": True, "narrow": 4}, ("cst_decode_loop_b16_s32.inc",)),
    ("gen_encode_loop_wide", {}, _names("cst_encode_loop_wide", "", "_sm")),
    ("gen_decode_loop_w16", {}, _names("cst_decode_loop_w16", "", "_sm")),
    ("gen_decode_loop_w16", {"packed": True}, ("cst_decode_loop_w16_pk.inc",)),
    ("gen_encode_loop_w16", {}, _names("cst_encode_loop_w16", "", "_sm")),
    ("gen_encode_loop_w16", {"packed": True}, ("cst_encode_loop_w16_pk.inc",)),
    ("gen_encode_loop_w16", {"packed": True, "ck": True}, ("cst_encode_loop_w16_pk_ck.inc",)),
    ("gen_pt_encode_loop", {}, ("cst_pt_encode_loop.inc",)),
    ("gen_pt_encode_loop", {"ck": True}, ("cst_pt_encode_loop_ck.inc",)),
    ("gen_pt_encode_loop", {"ck": True, "n8": True}, ("cst_pt_encode_loop_ck_n8.inc",)),
    ("gen_pt_decode_loop", {}, ("cst_pt_decode_loop.inc",)),
    ("gen_pt_decode_loop", {"sub": 1}, ("cst_pt_decode_loop_sub.inc",)),
    ("gen_pt_decode_loop", {"sub": 2}, ("cst_pt_decode_loop_sub16.inc",)),
    ("gen_pt_decode_loop", {"sub": 1, "n8": True}, ("cst_pt_decode_loop_sub_n8.inc",)),
    ("gen_pt_decode_loop", {"sub": 2, "n8": True}, ("cst_pt_decode_loop_sub16_n8.inc",)),
    ("gen_range_encode_loop", {}, _names("cst_range_encode_loop", "", "_2f", "_sm", "_2f_sm")),
    ("gen_range_encode_loop", {"ck": True}, _names("cst_range_encode_loop", "_ck", "_2f_ck")),
    ("gen_range_encode_loop", {"ck": True, "n8": True}, _names("cst_range_encode_loop", "_ck_n8", "_2f_ck_n8")),
    ("gen_range_decode_loop", {},
     _names("cst_range_decode_loop", "", "_ends", "_b16", "_b16_ends", "_sm", "_ends_sm", "_b16_sm", "_b16_ends_sm")),
    ("gen_range_decode_loop", {"sub": True}, _names("cst_range_decode_loop", "_sub", "_sub_ends", "_b16_sub", "_b16_sub_ends")),
    ("gen_range_decode_loop", {"sub": True, "n8": True},
     _names("cst_range_decode_loop", "_sub_n8", "_sub_n8_ends", "_b16_sub_n8", "_b16_sub_n8_ends")),
    ("gen_encode_loop_pc", {},
     _names("cst_encode_loop_pc", "", "_ck", "_w", "_w_ck", "_helper", "_loader", "_storer", "_storer2", "_n8", "_n8_ck",
            "_loader_n8", "_n16", "_n16_ck", "_loader_n16", "_n8w", "_n8w_ck", "_n16w", "_n16w_ck")),
)
FILES = tuple(name for _, _, files in LOOPS for name in files)
assert len(set(FILES)) == len(FILES)


@contextlib.contextmanager
def _environment(experiment):
    """no GEN_* variable reaches a generator unless this is an experiment run; nothing of one run's modules reaches the next"""
    saved, saved_path = dict(os.environ), list(sys.path)
    if not experiment:
        for name in [n for n in os.environ if n.startswith("GEN_")]:
            del os.environ[name]
    sys.path.insert(0, str(SCRIPTS))
    try:
        yield
    finally:
        sys.path[:] = saved_path                # (every generator puts scripts/ in front once more)
        os.environ.clear()
        os.environ.update(saved)


def run(generator, variant, files, experiment=False):
    """One manifest entry: executes the generator in a fresh namespace, hands it `variant`, returns {file name: text}.
    The run must make exactly the entry's files (an experiment may skip the forms it does not apply to, no more)."""
    for name in [n for n in sys.modules if n == "asmgen" or n.startswith("gen_")]:      # (generators import asmgen and each other)
        del sys.modules[name]
    spec = importlib.util.spec_from_file_location(generator, SCRIPTS / f"{generator}.py")
    mod = importlib.util.module_from_spec(spec)
    mod.__variant__ = dict(variant)
    spec.loader.exec_module(mod)
    if "__variant__" in vars(mod) and variant:
        raise TypeError(f"{generator} declares no variant knobs, got {', '.join(sorted(variant))}")
    texts = mod.main()
    if not set(texts) <= set(files) if experiment else sorted(texts) != sorted(files):
        raise RuntimeError(f"{generator} {variant}: made {sorted(texts)}, the manifest lists {sorted(files)}")
    return texts


def generate(only=None, experiment=False, verbose=False):
    """{file name: text} of every manifest entry (of generator `only`)"""
    entries = [e for e in LOOPS if only in (None, e[0])]
    if not entries:
        raise SystemExit(f"no generator {only}: " + " ".join(sorted({e[0] for e in LOOPS})))
    texts = {}
    with _environment(experiment), contextlib.redirect_stdout(sys.stdout if verbose else io.StringIO()):
        for entry in entries:
            texts.update(run(*entry, experiment))
    return texts


def stale(texts, directory):
    directory = Path(directory)
    return [name for name, text in texts.items()
            if not (directory / name).is_file() or (directory / name).read_bytes() != text.encode()]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="write nothing; list the stale files and fail if there are any")
    ap.add_argument("--out", type=Path, help="directory to generate into (or to check) instead of constriction_amd/csrc")
    ap.add_argument("--only", metavar="GENERATOR", help="only the runs of this generator")
    ap.add_argument("--experiment", action="store_true", help="let the GEN_* experiment knobs of the environment through (needs --out)")
    ap.add_argument("-v", "--verbose", action="store_true", help="instruction counts and wait notes of every statement")
    args = ap.parse_args(argv)
    out = (args.out or CSRC).resolve()
    if args.experiment and (args.check or out == CSRC.resolve()):
        ap.error("an experiment loop is wrong by design: generate it with --out DIR, never into constriction_amd/csrc")
    only = args.only and Path(args.only).stem
    texts = generate(only, args.experiment, args.verbose)
    changed = stale(texts, out)
    if not args.check:
        out.mkdir(parents=True, exist_ok=True)
        for name in changed:
            (out / name).write_bytes(texts[name].encode())
    for name in changed:
        print(("stale: " if args.check else "wrote ") + str(out / name))
    print(f"{len(texts)} files, {len(changed)} {'stale' if args.check else 'changed'}")
    return 1 if args.check and changed else 0


if __name__ == "__main__":
    sys.exit(main())
