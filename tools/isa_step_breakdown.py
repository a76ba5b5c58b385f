"""Per-step instruction breakdown of the column-segmented step loops, from the
gfx950 ISA (verdict round 4, item 4: instructions per step by role).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
        -fgpu-flush-denormals-to-zero -fdenormal-fp-math=preserve-sign \
        -munsafe-fp-atomics -fno-slp-vectorize --cuda-device-only -S \
        -o lane.s gatk-haplotypecaller-cpp17_amd/csrc/lane_kernel.hip
    python tools/isa_step_breakdown.py lane.s KERNEL_SUBSTRING [--json OUT]

LLVM annotates every loop member block with its header ("; in Loop:
Header=BBx_y"), so each step loop is the set of blocks sharing a header. A
plain step hands off 2 values by DPP (Y and the right-edge T; 4 DPP moves in
fp64) and does 11 (EQ path) or 12 (generic) mul/add per cell; a row-sum step
hands off 2 more and adds 2 per cell. The loop's kind, steps and block width
BC are the reading of its DPP and arithmetic counts that gives a compiled
width (8-64, even). Issue slots price each instruction at the rates measured on
gfx950 (tools/ubench/op_rate.hip, profiles/r02_op_rate_ubench.jsonl): 1 for
the full-rate forms, 2 for the half-rate ones (DPP, v_bfe, v_bitop3, v_cmp,
v_add_co, v_lshl_*, v_cndmask on an SGPR mask, f64 arithmetic, any VOP3 with
an SGPR operand). The prior select is v_add_co_u32 (the window shift, 2 slots)
and the e32 v_cndmask that reads its carry from VCC (1 slot; two per fp64
cell); s_nop (the VCC write-to-read wait states) is reported per step on its
own: it costs issue cycles of its wave, not VALU slots. The table path of the
fp32 EQ loops (seg_common.hpp cell_tab) has no select: per two columns one
shift of the window word, one v_and_or_b32 that puts its two bits into the
row's table base (priced as the other three-source forms, 2 slots) and the
ds_read_b64 of the pair, reported as "prior table (address)" and "prior table
(LDS read)". The quad form (fill_qtab) forms that address once per four columns
and reads 16 bytes at it (ds_read_b128, the priors of all four): a loop with
such reads is marked "quad". (Round 11's quad form read twice at the address,
ds_read_b64 with and without a DS immediate offset: both count as table reads,
and such a loop is marked "quad" as well.) The byte form (seg_spread.hpp) reads
a group's pattern byte from the spread window (ds_read_u8, a table read: no VALU
slot) and forms the address with one v_xor_b32 of that byte and the row's base
(full rate, 1 slot, "prior table (address)"): such a loop is marked "byte"."""
import collections
import json
import re
import sys

FULL = {"v_mul_f32", "v_add_f32", "v_sub_f32", "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32",
        "v_xor_b32", "v_not_b32", "v_lshrrev_b32", "v_ashrrev_i32", "v_mov_b32", "v_mov_b64"}


def writes_vcc(op, txt):
    """Whether the instruction's destination (or carry-out) is VCC."""
    args = [a.strip() for a in txt.split(None, 1)[1].split(",")] if " " in txt else []
    if not args:
        return False
    if "_co_" in op:
        return len(args) > 1 and args[1] == "vcc"
    return (op.startswith("v_cmp") or op.startswith("s_")) and args[0].startswith("vcc")


def operands(txt):
    return [a.strip() for a in txt.split(None, 1)[1].split(",")] if " " in txt else []


def table_roles(ins):
    """Indices of the prior table's instructions in a loop: every v_and_or_b32,
    the shift whose result it masks, and the ds_read_b64 or ds_read_b128 at its
    address (the address stays a table address until a VALU instruction
    overwrites its register: the two-read quad form read twice at it)."""
    addr, read = set(), set()
    shift_of, addr_regs, byte_regs = {}, set(), set()
    for i, (op, t) in enumerate(ins):
        a = operands(t)
        if op == "ds_read_u8":
            read.add(i)
            addr_regs.discard(a[0])
            byte_regs.add(a[0])
            continue
        if op == "v_xor_b32" and (a[1] in byte_regs or a[2] in byte_regs):
            addr.add(i)
            byte_regs.discard(a[0])
            addr_regs.add(a[0])
            continue
        if op == "v_and_or_b32":
            addr.add(i)
            if a[1] in shift_of:
                addr.add(shift_of.pop(a[1]))
            addr_regs.add(a[0])
            continue
        if op in ("ds_read_b64", "ds_read_b128") and a[1].split()[0] in addr_regs:   # "v165 offset:5120": the register
            read.add(i)
        if a and op.startswith("v_"):
            shift_of.pop(a[0], None)
            addr_regs.discard(a[0])
            byte_regs.discard(a[0])
            if op in ("v_lshrrev_b32", "v_lshlrev_b32"):
                shift_of[a[0]] = i
    return addr, read


def role(op, txt, vcc_is_carry=False):
    """vcc_is_carry: VCC was last written by a v_add_co_u32 (the window shift of
    prior_next), so an e32 v_cndmask reading it is the prior select's."""
    if op == "v_add_co_u32":
        return "prior select"
    if op == "v_cndmask_b32" and vcc_is_carry and txt.split()[0].endswith("_e32"):
        return "prior select"
    if "_dpp" in op or " wave_shr" in txt or "row_shr" in txt:
        return "handoff (DPP)"
    if op in ("v_mul_f32", "v_add_f32", "v_mul_f64", "v_add_f64"):
        return "cell arithmetic"
    if op in ("v_bfe_i32", "v_bitop3_b32", "v_bitop3_b16", "v_bfi_b32"):
        return "prior select"
    if op.startswith("v_cndmask") or op == "v_and_b32" and ("v" in txt.split(",")[-1] and "0x" not in txt):
        return "hand-off mask"
    if op.startswith("v_cmp") or op.startswith("s_"):
        return "row guard / loop (cmp, scalar)"
    if op.startswith("v_mov"):
        return "register moves"
    if op.startswith("global_") or op.startswith("ds_") or op.startswith("buffer_") or op.startswith("scratch_"):
        return "memory (read word, LDS priors, match row)"
    if op.startswith("v_"):
        return "row word / address arithmetic"
    return "other"


def slots(op, txt):
    if not op.startswith("v_"):
        return 0.0
    sgpr_operand = re.search(r"[ ,]s\[?\d", txt.split(op, 1)[1]) is not None
    if op in FULL and "_dpp" not in op and "_e64" not in txt.split()[0] and not sgpr_operand:
        return 1.0
    if op == "v_cndmask_b32" and txt.split()[0].endswith("_e32"):
        return 1.0
    return 2.0


def main():
    path, kname = sys.argv[1], sys.argv[2]
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\S*:", ln) and kname in ln)
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    loops = collections.defaultdict(list)   # header -> [(op, txt)]
    cur = None
    lab = None   # the last label: its loop-header note may follow on a comment line
    for ln in lines[start:end]:
        m = re.match(r"^\.(LBB\w+):\s*;?\s*(.*)$", ln)
        if m:
            lab, com = m.group(1), m.group(2)
            h = re.search(r"Header=(BB\w+)", com)
            if "Loop Header" in com:
                cur = lab[1:]
            elif h:
                cur = h.group(1)
            else:
                cur = None
            continue
        if lab is not None and re.match(r"^\s+;.*Loop Header", ln):
            # ".LBBx:  ; Parent Loop BBy" then ";  =>  This Inner Loop Header":
            # the label heads an inner loop (a one-block step loop has no
            # other member blocks, so without this it was missed).
            cur = lab[1:]
            continue
        if not ln.lstrip().startswith(";"):
            lab = None
        s = ln.strip()
        if cur is None or not s or s.startswith(";") or s.startswith("."):
            continue
        loops[cur].append((re.sub(r"_e(32|64)$", "", s.split()[0]), s))
    rows = []
    for hdr, ins in loops.items():
        c = collections.Counter(op for op, _ in ins)
        f32 = c["v_mul_f32"] + c["v_add_f32"]
        f64 = c["v_mul_f64"] + c["v_add_f64"]
        dpp = sum(1 for op, t in ins if "_dpp" in op)
        if dpp == 0 or (f32 < 100 and f64 < 100):
            continue
        fp64 = f64 > f32
        arith = f64 if fp64 else f32
        dpp_plain = 4 if fp64 else 2
        guess = None
        for sums, per_cell in ((False, 11), (False, 12), (True, 13), (True, 14)):
            steps = dpp // (dpp_plain * (2 if sums else 1))
            if steps and arith % (steps * per_cell) == 0:
                bc = arith // (steps * per_cell)
                if 8 <= bc <= 64 and bc % 2 == 0:
                    guess = (sums, steps, bc, per_cell == 11 or per_cell == 13)
                    break
        if guess is None:
            continue
        sums, steps, bc, eq = guess
        by_role = collections.Counter()
        by_slot = collections.Counter()
        carry = False
        tab_addr, tab_read = table_roles(ins)
        for i, (op, t) in enumerate(ins):
            r = role(op, t, carry)
            if i in tab_addr:
                r = "prior table (address)"
            elif i in tab_read:
                r = "prior table (LDS read)"
            by_role[r] += 1
            by_slot[r] += slots(op, t)
            if writes_vcc(op, t):
                carry = op == "v_add_co_u32"
        quad = any(op == "ds_read_b128" or "offset:" in t for i, (op, t) in enumerate(ins) if i in tab_read)
        byte = any(op == "ds_read_u8" for i, (op, t) in enumerate(ins) if i in tab_read)
        rows.append(dict(kernel=lines[start].split(":")[0], loop=hdr, fp64=fp64, bc=bc, eq=eq, quad=quad, byte=byte, row_sums=sums, steps_per_iteration=steps,
                         s_nop_per_step=round(c["s_nop"] / steps, 2),
                         select_ops_per_step={k: round(c[k] / steps, 2) for k in
                                              ("v_add_co_u32", "v_cndmask_b32", "v_bfe_i32", "v_bitop3_b32")},
                         table_ops_per_step={k: round(c[k] / steps, 2) for k in ("v_and_or_b32", "ds_read_b64", "ds_read_b128", "ds_read_u8")},
                         table_address_xor_per_step=round(sum(1 for i in tab_addr if ins[i][0] == "v_xor_b32") / steps, 2),
                         cndmask_e64_per_step=round(sum(1 for op, t in ins if op == "v_cndmask_b32"
                                                        and t.split()[0].endswith("_e64")) / steps, 2),
                         arith_per_step=arith / steps,
                         instr_per_step={k: round(v / steps, 2) for k, v in by_role.items()},
                         slots_per_step={k: round(v / steps, 2) for k, v in by_slot.items()},
                         total_instr_per_step=round(len(ins) / steps, 2),
                         valu_instr_per_step=round(sum(n for op, n in c.items() if op.startswith("v_")) / steps, 2),
                         valu_slots_per_step=round(sum(by_slot.values()) / steps, 2)))
    rows.sort(key=lambda r: (r["fp64"], not r["eq"], r["row_sums"], r["bc"], r["quad"]))
    for r in rows:
        print(json.dumps(r))
    if out_json:
        with open(out_json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
