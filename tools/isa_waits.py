#!/usr/bin/env python3
"""Developer tool (CPU only): where the vector-memory traffic of one step kernel sits and what its waits wait for.

On gfx950 global loads, global stores and scratch traffic share ONE in-order counter (vmcnt): `s_waitcnt vmcnt(N)` returns
once all but the newest N vector-memory instructions of the wavefront have completed, so a wait for a one-dword spill
reload also waits for every older store.  This tool compiles one unit of leibnizgym_amd/csrc/tf_env_kernels.hip with the
Makefile's flags to ISA (-S, -gline-tables-only for the source lines), takes one kernel out of it and models that counter
with a linear scan over the instruction stream.  It prints, per region between two s_barrier:
  - vector-memory loads / stores / scratch loads / scratch stores,
  - every vmcnt wait: what it retires (global loads, scratch loads, stores), how many instructions behind the newest
    load it sits, and the source line of that load,
  - chains load -> wait -> load -> wait (dependent round trips),
and for the whole kernel the loops that hold barriers with any vector-memory or scratch instruction inside them, the
scratch reloads in those loops that fetch what was stored in front of the loop (and whether that value was formed from
scalar registers and literals only: a constant of the launch parked in a spill slot), the spill / scratch figures of the
metadata, and the summary counts the tests/test_isa_*.py put caps on.

    python tools/isa_waits.py [--unit 0_0] [--kernel SUBSTR] [--full] [--no-min] [--asm FILE] [--keep FILE] [--json] [--quiet]

The scan is linear: it follows the text, not the control flow.  A wait behind a branch target is judged against what was
issued above it in the text, which is exact for straight-line code and for forward skips over code without vector-memory
traffic and an approximation elsewhere.  It is a tool for reading the ISA, not a proof.
"""
import argparse, collections, json, os, re, shutil, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "leibnizgym_amd", "csrc")
HEADLINE = "k_envILi9ELb0ELb1ELi127ELi0ELb0ELb0E"       # k_env<9, false, true, 127, 0, false, false>: bench.py's launch (unit 0_0)
NEAR = 8            # a wait at most this many instructions behind the load it is for hides nothing of its latency
CHAIN_GAP = 12      # two single-load waits belong to one chain if the second load issues within this many instructions of the first wait


def find_hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


def makefile_flags(unit):
    """CXXFLAGS + the -D flags of a unit, as the Makefile itself expands them"""
    out = subprocess.check_output(["make", "-s", "-C", CSRC, "--no-print-directory", "--eval",
                                   "isa-waits-flags: ; @echo $(CXXFLAGS) $(call unit_flags,%s)" % unit, "isa-waits-flags"], text=True)
    return out.split()


def compile_unit(unit, dev_min=True, keep=None):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    fd, path = tempfile.mkstemp(suffix=".s", prefix="isa_waits_")
    os.close(fd)
    cmd = [hipcc] + makefile_flags(unit) + (["-DTF_DEV_MIN"] if dev_min else []) + \
          ["-gline-tables-only", "--cuda-device-only", "-S", "-o", path, "tf_env_kernels.hip"]
    try:
        subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)
        text = open(path).read()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if keep:
        open(keep, "w").write(text)
    return text


Ins = collections.namedtuple("Ins", "idx op text kind loc labels")      # kind: gload gstore sload sstore atomic wait barrier other


def classify(op):
    if op.startswith("scratch_load"):
        return "sload"
    if op.startswith("scratch_store"):
        return "sstore"
    if re.match(r"(buffer|global|flat)_atomic", op):
        return "atomic"
    if re.match(r"(buffer|global|flat)_load", op):
        return "gload"
    if re.match(r"(buffer|global|flat)_store", op):
        return "gstore"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_barrier":
        return "barrier"
    return "other"


def extract_kernel(text, substr):
    """instructions, metadata of the first kernel whose mangled name holds substr"""
    lines = text.split("\n")
    start = name = None
    for n, l in enumerate(lines):
        m = re.match(r"^(_Z\S*):", l)
        if m and substr in m.group(1):
            start, name = n, m.group(1)
            break
    if start is None:
        raise RuntimeError("no kernel matching %r in the ISA" % substr)
    files, ins, loc, labels, meta = {}, [], None, [], {}
    for l in lines:          # file table of the .loc directives (whole translation unit)
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
    end = start
    for n in range(start + 1, len(lines)):
        l = lines[n]
        if l.startswith(".Lfunc_end"):
            end = n
            break
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            if int(m.group(2)) > 0:
                loc = "%s:%s" % (files.get(int(m.group(1)), "?"), m.group(2))
            continue
        m = re.match(r"^(\.L\w+):", l)
        if m:
            labels.append(m.group(1))
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        if not re.match(r"^(v_|s_|ds_|global_|buffer_|flat_|scratch_)", op):
            continue
        ins.append(Ins(len(ins), op, t, classify(op), loc, tuple(labels)))
        labels = []
    for l in lines[end:end + 60]:
        m = re.match(r";\s*(NumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
        if re.match(r"^_Z\S*:", l):
            break
    # spill counts: the .amdgpu_metadata entry of this kernel
    m = re.search(r"\.name:\s+%s\b(.*?)(?:\n\s+- \.a|\namdhsa\.|\Z)" % re.escape(name), text, re.S)
    blob = m.group(1) if m else ""
    pre = text[:m.start()] if m else ""
    for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
        # the fields of one entry sit on both sides of .name (alphabetical order): look back to the entry's start too
        back = pre[pre.rfind("\n  - ."):] if "\n  - ." in pre else ""
        mm = re.search(r"\.%s:\s*(\d+)" % key, back) or re.search(r"\.%s:\s*(\d+)" % key, blob)
        if mm:
            meta[key] = int(mm.group(1))
    return name, ins, meta


def vmcnt_of(text):
    m = re.search(r"vmcnt\((\d+)\)", text)
    if m:
        return int(m.group(1))
    m = re.match(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", text)      # raw immediate: vmcnt = bits 3:0 and 15:14
    if m:
        v = int(m.group(1), 0)
        return (v & 0xF) | ((v >> 14) & 0x3) << 4
    return None


def analyse(ins):
    """linear model of the vmcnt queue -> list of wait records, per-region counts, loops with barriers"""
    queue, waits, region = [], [], 0
    counts = collections.defaultdict(collections.Counter)
    for i in ins:
        if i.kind == "barrier":
            region += 1
            continue
        if i.kind in ("gload", "gstore", "sload", "sstore", "atomic"):
            counts[region][i.kind] += 1
            queue.append(i)
            continue
        if i.op == "s_endpgm":
            queue = []
            continue
        if i.kind != "wait":
            continue
        n = vmcnt_of(i.text)
        if n is None:
            continue
        retired = queue[:len(queue) - n] if n < len(queue) else []
        pending_loads = sum(r.kind in ("gload", "sload", "atomic") for r in queue)
        queue = queue[len(queue) - n:] if n else []
        if not retired:
            continue
        loads = [r for r in retired if r.kind in ("gload", "sload", "atomic")]
        stores = [r for r in retired if r.kind in ("gstore", "sstore")]
        rec = dict(idx=i.idx, region=region, n=n, loc=i.loc, pending_loads=pending_loads,
                   gloads=sum(r.kind == "gload" for r in retired), sloads=sum(r.kind == "sload" for r in retired),
                   atomics=sum(r.kind == "atomic" for r in retired),
                   gstores=sum(r.kind == "gstore" for r in retired), sstores=sum(r.kind == "sstore" for r in retired))
        if loads:
            newest = loads[-1]
            rec.update(dist=i.idx - newest.idx, load_idx=newest.idx, load_loc=newest.loc, load_kind=newest.kind, load_text=newest.text,
                       first_load_idx=loads[0].idx,
                       # a store is "covered" when it is older than a load the wait is for: the load's data cannot be used before the store has completed
                       covered_gstores=sum(r.kind == "gstore" and r.idx < newest.idx for r in retired))
        waits.append(rec)
    # chains of single-load waits: load -> wait -> load -> wait ...
    # single-load wait: ONE load in flight (not the last step of a vmcnt(2) / (1) / (0) stair over loads issued together), waited for within NEAR
    # instructions of its issue: a full round trip that hides nothing
    single = [w for w in waits if w.get("load_idx") is not None and w["pending_loads"] == 1 and w["dist"] <= NEAR]
    chains, cur = [], []
    for w in single:
        if cur and w["load_idx"] > cur[-1]["idx"] and w["load_idx"] - cur[-1]["idx"] <= CHAIN_GAP and \
           not any(x.kind in ("gload", "sload", "gstore", "sstore", "atomic", "barrier") for x in ins[cur[-1]["idx"] + 1:w["load_idx"]]):
            cur.append(w)
        else:
            if len(cur) >= 2:
                chains.append(cur)
            cur = [w]
    if len(cur) >= 2:
        chains.append(cur)
    return waits, single, chains, counts, find_loops(ins)


def find_loops(ins):
    """natural loops of the control-flow graph that hold at least one barrier (block placement makes a backward branch in the text
    no evidence of a loop: back edges are the edges into a dominator)"""
    where = {}
    for i in ins:
        for lb in i.labels:
            where[lb] = i.idx
    leaders = {0}
    for i in ins:
        if i.labels:
            leaders.add(i.idx)
        if i.op.startswith(("s_cbranch", "s_branch")) or i.op == "s_endpgm":
            leaders.add(i.idx + 1)
    starts = sorted(x for x in leaders if x < len(ins))
    block_of = {}
    for b, s0 in enumerate(starts):
        for k in range(s0, starts[b + 1] if b + 1 < len(starts) else len(ins)):
            block_of[k] = b
    nb = len(starts)
    ends = [(starts[b + 1] if b + 1 < nb else len(ins)) - 1 for b in range(nb)]
    succ = [[] for _ in range(nb)]
    for b in range(nb):
        last = ins[ends[b]]
        if last.op == "s_endpgm":
            continue
        if last.op.startswith(("s_cbranch", "s_branch")):
            tgt = last.text.split()[-1]
            if tgt in where:
                succ[b].append(block_of[where[tgt]])
            if last.op.startswith("s_branch"):
                continue
        if b + 1 < nb:
            succ[b].append(b + 1)
    pred = [[] for _ in range(nb)]
    for b in range(nb):
        for t in succ[b]:
            pred[t].append(b)
    # loops = strongly connected components, nested ones found by taking a component's entry blocks out and looking again (block placement makes
    # a backward branch in the text no evidence of a loop, and the sweep loops have two entries: no single header dominates them)
    def sccs(nodes):
        index, low, onst, st, out, n = {}, {}, set(), [], [], 0
        for root in sorted(nodes):
            if root in index:
                continue
            work = [(root, iter(succ[root]))]
            index[root] = low[root] = n; n += 1; st.append(root); onst.add(root)
            while work:
                v, it = work[-1]
                for t in it:
                    if t not in nodes:
                        continue
                    if t not in index:
                        index[t] = low[t] = n; n += 1; st.append(t); onst.add(t)
                        work.append((t, iter(succ[t])))
                        break
                    if t in onst:
                        low[v] = min(low[v], index[t])
                else:
                    work.pop()
                    if work:
                        low[work[-1][0]] = min(low[work[-1][0]], low[v])
                    if low[v] == index[v]:
                        comp = set()
                        while True:
                            x = st.pop(); onst.discard(x); comp.add(x)
                            if x == v:
                                break
                        if len(comp) > 1 or v in succ[v]:
                            out.append(comp)
        return out
    bodies, todo = [], [set(range(nb))]
    while todo:
        for comp in sccs(todo.pop()):
            entries = {x for x in comp if x == 0 or any(p not in comp for p in pred[x])} or {min(comp)}
            bodies.append((min(entries), comp))
            if len(comp) > len(entries):
                todo.append(comp - entries)
    loops = []
    for h, body in bodies:
        code = [ins[k] for b in sorted(body) for k in range(starts[b], ends[b] + 1)]
        nbar = sum(x.kind == "barrier" for x in code)
        if nbar:
            loops.append(dict(first=starts[h], label=(ins[starts[h]].labels or ("?",))[-1], blocks=body, barriers=nbar, size=len(code),
                              vmem=[x for x in code if x.kind in ("gload", "gstore", "atomic")],
                              scratch=[x for x in code if x.kind in ("sload", "sstore")]))
    for lp in loops:      # innermost: no other barrier loop strictly inside
        lp["innermost"] = not any(o is not lp and o["blocks"] < lp["blocks"] for o in loops)
    loops.sort(key=lambda lp: lp["first"])
    return loops


def summary(name, ins, meta, waits, single, chains, loops):
    sweep = [lp for lp in loops if lp["innermost"] and lp["barriers"] >= 2]
    return {
        "kernel": name,
        "instructions": len(ins),
        "vgprs": meta.get("NumVgprs"), "occupancy": meta.get("Occupancy"),
        "vgpr_spills": meta.get("vgpr_spill_count"), "sgpr_spills": meta.get("sgpr_spill_count"),
        "scratch_bytes": meta.get("ScratchSize", meta.get("private_segment_fixed_size")),
        "barriers": sum(i.kind == "barrier" for i in ins),
        "global_loads": sum(i.kind == "gload" for i in ins), "global_stores": sum(i.kind == "gstore" for i in ins),
        "scratch_loads": sum(i.kind == "sload" for i in ins), "scratch_stores": sum(i.kind == "sstore" for i in ins),
        "vmcnt_waits": len(waits),
        "single_load_waits": len(single),
        "single_load_waits_scratch": sum(w["load_kind"] == "sload" for w in single),
        "single_load_waits_global": sum(w["load_kind"] != "sload" for w in single),
        "store_covering_waits": sum(1 for w in waits if w.get("covered_gstores", 0) > 0),
        "chains": len(chains),
        "longest_chain": max([len(c) for c in chains], default=0),
        "state_row_chains": sum(1 for c in chains if sum(w["load_kind"] == "gload" for w in c) >= 2),
        "longest_state_row_chain": max([max_run(c) for c in chains], default=0),
        "sweep_loops": len(sweep),
        "sweep_loop_vmem": sum(len(lp["vmem"]) for lp in sweep),
        "sweep_loop_scratch": sum(len(lp["scratch"]) for lp in sweep),
    }


def max_run(chain):
    """longest run of consecutive global-load links in a chain"""
    best = run = 0
    for w in chain:
        run = run + 1 if w["load_kind"] == "gload" else 0
        best = max(best, run)
    return best if best >= 2 else 0


def loop_code(ins, lp):
    """the instructions of a loop of find_loops, in text order"""
    leaders = {0}
    for i in ins:
        if i.labels:
            leaders.add(i.idx)
        if i.op.startswith(("s_cbranch", "s_branch")) or i.op == "s_endpgm":
            leaders.add(i.idx + 1)
    starts = sorted(x for x in leaders if x < len(ins))
    out = []
    for b in sorted(lp["blocks"]):
        out += ins[starts[b]:(starts[b + 1] if b + 1 < len(starts) else len(ins))]
    return out


def _regs(tok):
    """registers an operand names: ("v", {numbers}) / ("s", ...) / None for literals, inline constants, vcc, exec, off, modifiers"""
    tok = tok.strip().lstrip("-|").rstrip("|")
    m = re.match(r"^([vsa])(\d+)$", tok)
    if m:
        return m.group(1), {int(m.group(2))}
    m = re.match(r"^([vsa])\[(\d+):(\d+)\]$", tok)
    if m:
        return m.group(1), set(range(int(m.group(2)), int(m.group(3)) + 1))
    return None


def _operands(text):
    body = text.split(None, 1)[1] if " " in text else ""
    return [t for t in re.split(r",\s*(?![^\[]*\])", body) if t]


def scratch_slot(i):
    """(first byte, bytes) of the scratch slot a scratch_load / scratch_store touches"""
    m = re.search(r"offset:(\d+)", i.text)
    w = re.search(r"dwordx(\d)", i.op)
    return (int(m.group(1)) if m else 0), 4 * (int(w.group(1)) if w else 1)


ACCUMULATING = ("v_fmac", "v_mac", "v_pk_fmac", "v_dot")      # the destination is a source too
MAX_TRACE = 600


def wave_uniform(ins, at, reg, depth=0):
    """Is VGPR `reg`, as instruction `at` reads it, formed from scalar registers and literals only?  A backward walk over the text (like the rest of this
    tool it follows the text, not the control flow): the nearest earlier instruction that writes the register decides - a vector-ALU instruction whose sources
    are SGPRs, literals or VGPRs that are themselves uniform.  Anything else (a load, a lane instruction, a select, no definition inside the basic block) counts
    as per lane."""
    if depth > 12:
        return False
    for k in range(at - 1, max(at - MAX_TRACE, -1), -1):
        i = ins[k]
        if ins[k + 1].labels or re.search(r"\bexec\b", i.text.split(",")[0]) or i.op.startswith(("s_cbranch", "s_branch")):
            return False                                     # the walk stays inside one basic block with one EXEC mask: a write further up may have been a partial one
        ops = _operands(i.text)
        if not ops or not i.op.startswith("v_"):
            d = _regs(ops[0]) if ops else None
            if d and d[0] == "v" and reg in d[1] and not i.op.startswith(("scratch_store", "global_store", "buffer_store", "flat_store", "ds_write")):
                return False                                 # written by a load
            continue
        d = _regs(ops[0])
        if not (d and d[0] == "v" and reg in d[1]):
            continue
        if i.op.startswith(("v_cndmask", "v_mbcnt", "v_writelane", "v_readlane", "v_readfirstlane", "v_permlane", "v_mov_b32_dpp", "v_div_fmas", "v_accvgpr")) and not i.op.startswith("v_div_fmas"):
            return False
        srcs = ops[1:]
        if i.op.startswith("v_div_scale"):                   # two destinations: the value and a scalar mask
            srcs = ops[2:]
        if i.op.startswith(ACCUMULATING):
            srcs = srcs + [ops[0]]
        for t in srcs:
            r = _regs(t)
            if r is None or r[0] == "s":
                continue
            if r[0] != "v" or not all(wave_uniform(ins, k, x, depth + 1) for x in r[1]):
                return False
        return True
    return False


def loop_reloads(ins, lp):
    """every scratch reload inside loop lp whose slot is stored in front of the loop: the store, and whether the stored value is wave-uniform"""
    code = loop_code(ins, lp)
    inside = {i.idx for i in code}
    first = min(inside)
    out = []
    for ld in code:
        if ld.kind != "sload":
            continue
        lo, n = scratch_slot(ld)
        stores = []
        for st in ins[:first]:
            if st.kind == "sstore" and st.idx not in inside:
                slo, sn = scratch_slot(st)
                if slo < lo + n and lo < slo + sn:
                    stores.append(st)
        if not stores or any(st.kind == "sstore" and scratch_slot(st)[0] < lo + n and lo < sum(scratch_slot(st)) for st in code):
            continue                                         # stored inside the loop (or nowhere in front of it): not a value parked in front of the loop
        st = stores[-1]                                      # the last store in front of the loop is the one the loop finds
        r = _regs(_operands(st.text)[1])
        uniform = bool(r) and r[0] == "v" and all(wave_uniform(ins, st.idx, x) for x in r[1])
        out.append(dict(load=ld, store=st, slot=lo, bytes=n, uniform=uniform))
    return out


def barrier_loop_reloads(ins, loops):
    """loop_reloads of every loop that holds barriers (an inner loop's reloads are its outer loop's too: counted once, by instruction)"""
    seen, out = set(), []
    for lp in loops:
        for r in loop_reloads(ins, lp):
            if r["load"].idx not in seen:
                seen.add(r["load"].idx)
                out.append(dict(r, loop=lp["label"]))
    return out


def run(unit="0_0", kernel=HEADLINE, dev_min=True, asm=None, keep=None):
    if unit.startswith("d") and kernel.startswith("k_envI"):      # the d0_* and d2_* units (domain randomisation as a run-time flag): the same kernels, named k_env_dr
        kernel = "k_env_dr" + kernel[len("k_env"):]
    text = open(asm).read() if asm else compile_unit(unit, dev_min, keep)
    name, ins, meta = extract_kernel(text, kernel)
    waits, single, chains, counts, loops = analyse(ins)
    reloads = barrier_loop_reloads(ins, loops)
    s = summary(name, ins, meta, waits, single, chains, loops)
    s["barrier_loop_scratch_max"] = max([len(lp["scratch"]) for lp in loops], default=0)      # most scratch instructions in one loop that holds barriers
    s["loop_reloads_of_preloop_stores"] = len(reloads)                                       # scratch reloads in such loops of values stored in front of the loop
    s["loop_reloads_of_preloop_uniform"] = sum(r["uniform"] for r in reloads)                # ... of values formed from scalar registers and literals only
    return dict(name=name, ins=ins, meta=meta, waits=waits, single=single, chains=chains, counts=counts, loops=loops, reloads=reloads, summary=s)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", default="0_0", help="translation unit of the Makefile (0_0, d0_0, 1_2, s0_1, ...)")
    ap.add_argument("--kernel", default=HEADLINE, help="substring of the mangled kernel name (default: the headline launch)")
    ap.add_argument("--no-min", action="store_true", help="compile without -DTF_DEV_MIN (every instantiation of the unit: slower)")
    ap.add_argument("--asm", help="read this ISA file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled ISA in this file")
    ap.add_argument("--full", action="store_true", help="list every wait, not only the single-load and the store-covering ones")
    ap.add_argument("--json", action="store_true", help="print the summary as one JSON line only")
    ap.add_argument("--quiet", action="store_true", help="summary only")
    a = ap.parse_args()
    r = run(a.unit, a.kernel, not a.no_min, a.asm, a.keep)
    s = r["summary"]
    if a.json:
        print(json.dumps(s))
        return
    print("kernel %s (unit %s)" % (r["name"], a.unit))
    print("  %d instructions, %d barriers; VGPRs %s, occupancy %s; spills %s VGPR / %s SGPR, scratch %s B" %
          (s["instructions"], s["barriers"], s["vgprs"], s["occupancy"], s["vgpr_spills"], s["sgpr_spills"], s["scratch_bytes"]))
    if not a.quiet:
        ins, by_region = r["ins"], collections.defaultdict(list)
        for w in r["waits"]:
            by_region[w["region"]].append(w)
        single_ids = {w["idx"] for w in r["single"]}
        print("\nregions (between barriers): global loads / global stores / scratch loads / scratch stores, then the waits")
        for reg in range(s["barriers"] + 1):
            c = r["counts"].get(reg, {})
            ws = by_region.get(reg, [])
            if not ws and not any(c.values()) if c else not ws:
                continue
            print("region %2d: gload %3d  gstore %3d  sload %3d  sstore %3d  atomic %d   vmcnt waits %d" %
                  (reg, c.get("gload", 0), c.get("gstore", 0), c.get("sload", 0), c.get("sstore", 0), c.get("atomic", 0), len(ws)))
            for w in ws:
                tag = ("single " if w["idx"] in single_ids else "") + ("covers-stores " if w.get("covered_gstores") else "")
                if not (a.full or tag):
                    continue
                print("    @%6d vmcnt(%d): retires %d global + %d scratch loads, %d atomics, %d global + %d scratch stores%s  %s" %
                      (w["idx"], w["n"], w["gloads"], w["sloads"], w["atomics"], w["gstores"], w["sstores"],
                       ("; %d instr behind newest load (%s)" % (w["dist"], w["load_loc"])) if "dist" in w else "", tag))
        print("\nchains load -> wait -> load -> wait (every link a full round trip):")
        for c in r["chains"]:
            print("    %d links from @%d: %s" % (len(c), c[0]["load_idx"], ", ".join("%s %s" % (w["load_kind"], w["load_loc"]) for w in c)))
        print("\nloops that hold barriers:")
        for lp in r["loops"]:
            print("    %s @%d: %d instructions, %d barriers%s, vector-memory %d, scratch %d" %
                  (lp["label"], lp["first"], lp["size"], lp["barriers"], " (innermost)" if lp["innermost"] else "", len(lp["vmem"]), len(lp["scratch"])))
            if lp["innermost"]:
                for x in lp["vmem"] + lp["scratch"]:
                    print("        @%d %s   %s" % (x.idx, x.text, x.loc))
        print("\nscratch reloads inside loops that hold barriers of values stored in front of the loop (uniform: formed from scalar registers and literals only):")
        for x in r["reloads"]:
            print("    slot %3d (%d B) %-8s stored @%d %s, reloaded @%d %s in %s" % (x["slot"], x["bytes"], "uniform" if x["uniform"] else "per lane",
                  x["store"].idx, x["store"].loc, x["load"].idx, x["load"].loc, x["loop"]))
    print("\nsummary")
    for k, v in s.items():
        if k != "kernel":
            print("  %-28s %s" % (k, v))


if __name__ == "__main__":
    sys.exit(main())
