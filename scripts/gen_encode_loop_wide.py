#!/usr/bin/env python3
"""Generates constriction_amd/csrc/cst_encode_loop_wide.inc: the hand-scheduled gfx950 main loop of the (32,64) ANS encoder
for 12 < P <= 24 (DefaultAnsCoder's PRECISION = 24) -- gen_encode_loop.py's pipeline and step on UNPACKED table entries
{c, p, floor(2^64 / p)} (the half-word selects of the P <= 12 form do not fit 24-bit probabilities: three more
instructions per step derive p << (32 - P), 2^P - p and c + 2^P - p), with two word groups leaving per tile (32 symbols
can emit 24 words) as in gen_encode_loop_w16.py.

Run:  python scripts/gen_encode_loop_wide.py   (rewrites the .inc; the .inc is checked in)
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_encode_loop as G  # noqa: E402
import gen_encode_loop_w16 as W  # noqa: E402
from asmgen import Asm, Statements  # noqa: E402

A0, A1, W0, W1, U0, U1, T0, T1, SM0, SM1, Q0, Q1 = G.A0, G.A1, G.W0, G.W1, G.U0, G.U1, G.T0, G.T1, G.SM0, G.SM1, G.Q0, G.Q1
A_T, W_T, U_T, T_T, SM_T, Q_T = G.A_T, G.W_T, G.U_T, G.T_T, G.SM_T, G.Q_T
RR, PSHL, CK, RA, SD, LO, HI, ST_T = G.RR, G.PSHL, G.CK, G.RA, G.SD, G.LO, G.HI, G.ST_T


def step(a, c, p, m0, m1):
    """stack.rs:1035-1045 exactly as gen_encode_loop.step, operands derived from c and p in full registers:
    24 VALU instructions + the ring write.  The new state is q_est 2^P + r + c + (fix ? 2^P : 0) with r = min(r_est, r_est - p)
    (the smaller of the two as unsigned numbers: r_est - p wraps if r_est < p) -- one 64-bit mad on [r + c + fix 2^P, q_est_hi << P]."""
    a.i(f"v_lshlrev_b32 {PSHL}, %[sh], {p}", "p << (32 - P)")
    a.i(f"v_cmp_ge_u32 vcc, {HI}, {PSHL}", "emit <=> (state >> (64 - P)) >= p")
    a.i(f"v_lshlrev_b32 {RA}, 8, %[wr]")
    a.i(f"v_and_or_b32 {RA}, {RA}, %[c3f00], %[lanebase]")
    a.i(f"v_cndmask_b32_e64 {A0}, {LO}, {HI}, vcc")
    a.i(f"v_cndmask_b32_e64 {A1}, {HI}, 0, vcc")
    a.ds(f"ds_write_b32 {RA}, {LO}", "W", "candidate word, always written")
    a.i(f"v_addc_co_u32 %[wr], vcc, 0, %[wr], vcc")
    a.i(f"v_mul_hi_u32 {W0}, {A0}, {m0}")
    a.i(f"v_mad_u64_u32 {U_T}, vcc, {A1}, {m0}, {W_T}", "U = a1*m0 + hi32(a0*m0)   (< 2^64)")
    a.i(f"v_mad_u64_u32 {T_T}, vcc, {A0}, {m1}, {U_T}", "T = a0*m1 + U, carry -> vcc")
    a.i(f"v_mov_b32 {SM0}, {T1}")
    a.i(f"v_addc_co_u32 {SM1}, vcc, 0, {W1}, vcc", "[T_hi, carry]")
    a.i(f"v_mad_u64_u32 {Q_T}, vcc, {A1}, {m1}, {SM_T}", "q_est in {q - 1, q}")
    a.i(f"v_mul_lo_u32 {RR}, {Q0}, {p}")
    a.i(f"v_sub_u32 {RR}, {A0}, {RR}", "r_est (< 2p: its low 32 bits)")
    a.i(f"v_sub_u32 {CK}, {RR}, {p}", "r_est - p   (wraps if r_est < p)")
    a.i(f"v_cmp_ge_u32 vcc, {RR}, {p}", "fix <=> q = q_est + 1")
    a.i(f"v_min_u32 {RR}, {RR}, {CK}", "r")
    a.i(f"v_cndmask_b32 {CK}, 0, %[twoP], vcc", "fix 2^P")
    a.i(f"v_lshlrev_b32 {A1}, %[P], {Q1}", "q_est_hi << P   (q < 2^(64 - P))")
    a.i(f"v_add3_u32 {A0}, {RR}, {c}, {CK}", "r + c + fix 2^P   (< 2^26)")
    a.i(f"v_mad_u64_u32 {ST_T}, {SD}, {Q0}, %[twoP], {A_T}", "state = q_est 2^P + r + c + fix 2^P")


def main():
    out = Statements(__file__)
    emit(out, "cst_encode_loop_wide.inc", False)
    emit(out, "cst_encode_loop_wide_sm.inc", True)              # symbols[t][stream]: gen_encode_loop.py's SYMBOL_MAJOR staging
    return out


def emit(out, name, symbol_major):
    W.step = step                     # the (16,32) generator's tile body (two word groups per tile) around this step
    G.SINGLE = False
    G.SYMBOL_MAJOR = symbol_major
    a = Asm()
    a.i(f"v_mov_b32 {W1}, 0")
    a.i(f"v_mov_b32 {LO}, %[lo]")
    a.i(f"v_mov_b32 {HI}, %[hi]")
    a.i("s_mov_b64 s[80:81], %[sbase]", "symbols of the LAST full tile of stream s0")
    a.i("s_mov_b32 s82, %[ntiles]", "tiles left to encode")
    a.i("s_sub_u32 s83, %[ntiles], 1", "tiles left to request")
    G.load_set(a, "A")
    G.load_set(a, "B")
    G.stage_set(a, "A", 0)
    G.load_set(a, "A")
    G.read_syms(a, 0, 0, 7)
    G.read_syms(a, 1, 0, 6)
    a.wait_lds("S0")
    G.fetch_entries(a, 0)
    a.i("1:")
    first = len(a.events)
    W.half(a, 0, 0)
    a.i("s_sub_u32 s82, s82, 1")
    a.i("s_cmp_eq_u32 s82, 0")
    a.i("s_cbranch_scc1 2f")
    W.half(a, 1, 8)
    a.i("s_sub_u32 s82, s82, 1")
    a.i("s_cmp_lg_u32 s82, 0")
    a.i("s_cbranch_scc1 1b")
    ren = {"S16": "S0", "S17": "S1", "E16": "E0"}
    lds_back = [ren.get(t, t) for t in a.lds]
    lds_end, vm_end, notes = a.verify_loop(first, lds_back, a.vm, passes=1)
    lds_end = [ren.get(t, t) for t in lds_end]
    assert lds_end == lds_back, (lds_end, lds_back)
    a.i("2:")
    a.i(f"v_mov_b32 %[lo], {LO}")
    a.i(f"v_mov_b32 %[hi], {HI}")
    a.wait_vm_all("nothing may land in the scratch registers after the statement")
    a.wait_lds_all()
    about = ["// Main loop of the hand-scheduled (32,64) ANS encoder for 12 < P <= 24: see cst_ans_b16.hip."]
    ops = ['    : [lo] "+v"(lo), [hi] "+v"(hi), [wr] "+v"(wr), [flushed] "+v"(flushed), [smin] "+v"(smin), [smax] "+v"(smax)',
           '    : [row0] "v"(tile_row_addr[0]), [row1] "v"(tile_row_addr[1]), [tr0] "v"(tile_tr_addr[0]), [tr1] "v"(tile_tr_addr[1]),',
           '      [lanebase] "v"(ring_lane_addr), [cap] "v"(cap), [slaboff] "v"(slab_off),',
           '      [tbl] "s"(table_addr_biased), [twoP] "v"(1u << P), [P] "s"(P), [sh] "s"(32u - P), [c3f00] "s"(0x3f00u), [wbase] "s"(words_base),',
           '      [sbase] "s"(symbols_base), [ntiles] "s"(n_tiles),' + (' [tilestep] "s"(tile_step_bytes),' if symbol_major else ''),
           '      ' + ", ".join(f'[goff{k}] "v"(goff[{k}])' for k in range(8)),
           "    : " + ", ".join(f'"{c}"' for c in G.CLOBBERS) + ");"]
    out.add(name, a, about, ops, notes=notes)
    G.SYMBOL_MAJOR = False


if __name__ == "__main__":
    import loops
    raise SystemExit(loops.main(["--only", "gen_encode_loop_wide"]))
