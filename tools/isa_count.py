#!/usr/bin/env python3
"""Trip-weighted static instruction counts of the two ladder kernels, taken from the SHIPPED code object.

    python tools/isa_count.py [path/to/libsecp256k1_voi_amd.so]      -> JSON on stdout

The library's gfx950 code objects are unbundled with `llvm-objdump --offloading`, the kernel is disassembled with
`llvm-objdump -d`, and the loops are recovered from the control-flow graph of the disassembly (basic blocks; a loop is a
strongly connected component, the loops inside it are the components left when the edges into its entries are cut - the
code layout does not matter, nor does a second entry into a loop).  Trip counts are
those of the source:

  k_verify_fast<ECDSA>        table forward 7 | table backward 7 | ladder 32 x (doubling loop 4, addition loop 2) | generator part GT_WINDOWS - 1
                              (the last generator addition stands outside the loop)
  k_verify_fast<ECDSA_KEYED>  main loop of 4 rounds, entered past its first blocks (the change of form and the doubling loop
                              run between rounds only: 3 times; doubling loop 4 per time), chunk loop 8, addition loop 2
  k_verify_fast<ECDSA_COMB>   round loop 19: a column (two additions, the entries added to each other first), the exit test,
                              the doubling (18)
  k_verify_fast<SCHNORR_KEYED> / <SCHNORR_COMB>   the BIP-340 ladders over the same tables: the loops of ECDSA_KEYED / ECDSA_COMB
  k_verify_comb<false> / <true>   the comb ladders without the lead point (comb_ladder.hip; the default of ECDSA and BIP-340 calls): the
                              first round peeled in front of the loop, round loop 18: the doubling, then a column (18 / 18)
  k_verify_row                table 7 | 32 windows x (doubling loop 4, two additions) | generator part GT_WINDOWS      (a wave per signature)
  k_verify_row_keyset / k_schnorr_row_keyset   chunk loop 32 (two additions each) | generator part GT_WINDOWS      (the same over a key set)
  k_verify_row_comb / k_schnorr_row_comb       column 18 in front of the loop | round loop 18 (a doubling, two additions) | generator part
                              GT_WINDOWS      (the same over a comb key set)

This is what ties the roofline's instruction counts (profiles/r04_valu_counts.json, PMC) to the binary that is measured:
tests/test_counts_cpu.py recounts the built library and compares, bench.py recounts the library it loaded.
(tools/isa_mix.py / isa_mix_keyed.py do the same on the compiler's assembly listing, with its loop comments; they need a
two-minute compile, this needs none.)"""
import json
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "secp256k1_voi_amd", "libsecp256k1_voi_amd.so")


def code_objects(lib):
    """Unbundles the gfx950 code objects of `lib` into a temporary directory; returns (tmpdir, [paths])."""
    tmp = tempfile.mkdtemp(prefix="s2k_isa_")
    work = os.path.join(tmp, "lib.so")
    os.symlink(os.path.abspath(lib), work)
    subprocess.run([OBJDUMP, "--offloading", work], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return tmp, sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f)


def disassemble_symbol(obj, name):
    """[(offset, opcode, branch_target_offset or None)] of the function `name` of the code object `obj`."""
    out = subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + name, obj], capture_output=True, text=True, check=True).stdout
    ins, base = [], None
    for l in out.splitlines():
        m = re.match(r"^\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):", l) or re.match(r"^\s+(\S+)\s*//\s*([0-9A-Fa-f]+):", l)
        if not m:
            continue
        addr = int(m.group(2), 16)
        if base is None:
            base = addr
        tgt = None
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$", l)
            tgt = int(t.group(1), 16) if t else 0      # (no offset: the kernel's first instruction)
        ins.append((addr - base, m.group(1), tgt))
    return ins


def disassemble(lib, mangled_prefix):
    """disassemble_symbol of the kernel whose mangled name starts with `mangled_prefix`."""
    tmp, objs = code_objects(lib)
    try:
        for obj in objs:
            syms = subprocess.run([OBJDUMP, "-t", obj], capture_output=True, text=True, check=True).stdout
            names = [l.split()[-1] for l in syms.splitlines() if l.split() and l.split()[-1].startswith(mangled_prefix) and " F " in l]
            names = [n for n in names if not n.endswith(".kd")]
            if names:
                return disassemble_symbol(obj, names[0])
        raise RuntimeError("kernel %s* not found in %s" % (mangled_prefix, lib))
    finally:
        subprocess.run(["rm", "-rf", tmp])


def has_kernel(lib, mangled_prefix):
    try:
        disassemble(lib, mangled_prefix)
        return True
    except RuntimeError:
        return False


class Cfg:
    """Basic blocks, dominators and natural loops of one kernel's disassembly."""

    def __init__(self, ins):
        self.ins = ins
        offs = [o for o, _, _ in ins]
        index = {o: i for i, o in enumerate(offs)}
        leaders = {0}
        for i, (off, op, tgt) in enumerate(ins):
            if tgt is not None:
                leaders.add(index[tgt])
                if i + 1 < len(ins):
                    leaders.add(i + 1)
            elif op.startswith(("s_endpgm", "s_setpc", "s_swappc")) and i + 1 < len(ins):
                leaders.add(i + 1)
        starts = sorted(leaders)
        self.blocks = [(starts[k], starts[k + 1] if k + 1 < len(starts) else len(ins)) for k in range(len(starts))]
        self.block_of = {}
        for b, (lo, hi) in enumerate(self.blocks):
            for i in range(lo, hi):
                self.block_of[i] = b
        nb = len(self.blocks)
        self.succ = [[] for _ in range(nb)]
        for b, (lo, hi) in enumerate(self.blocks):
            off, op, tgt = ins[hi - 1]
            if tgt is not None:
                self.succ[b].append(self.block_of[index[tgt]])
            if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and hi < len(ins):
                self.succ[b].append(self.block_of[hi])
        self.pred = [[] for _ in range(nb)]
        for b in range(nb):
            for t in self.succ[b]:
                self.pred[t].append(b)
        # Loop forest from strongly connected components (works for loops with two entries too - the keyed ladder's round
        # loop is entered past its first blocks AND, by a never-taken guard, at them): a nontrivial SCC is a loop; its
        # entries are the blocks with a predecessor outside; with the edges into the entries cut, the SCCs inside are the
        # nested loops.
        self.loops = []                                   # dicts: blocks (set), entries (sorted list), parent (index or None)
        self._nest(set(range(nb)), set(), None)

    def _sccs(self, nodes, cut):
        """nontrivial SCCs of the graph on `nodes` without the edges into `cut` (Tarjan, iterative)"""
        idx, low, on, stack, out, counter = {}, {}, set(), [], [], [0]
        for root in sorted(nodes):
            if root in idx:
                continue
            work = [(root, iter([t for t in self.succ[root] if t in nodes and t not in cut]))]
            idx[root] = low[root] = counter[0]
            counter[0] += 1
            stack.append(root)
            on.add(root)
            while work:
                v, it = work[-1]
                advanced = False
                for t in it:
                    if t not in idx:
                        idx[t] = low[t] = counter[0]
                        counter[0] += 1
                        stack.append(t)
                        on.add(t)
                        work.append((t, iter([x for x in self.succ[t] if x in nodes and x not in cut])))
                        advanced = True
                        break
                    elif t in on:
                        low[v] = min(low[v], idx[t])
                if advanced:
                    continue
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == idx[v]:
                    comp = set()
                    while True:
                        x = stack.pop()
                        on.discard(x)
                        comp.add(x)
                        if x == v:
                            break
                    if len(comp) > 1 or v in [t for t in self.succ[v] if t not in cut]:
                        out.append(comp)
        return out

    def _nest(self, nodes, cut, parent):
        for comp in sorted(self._sccs(nodes, cut), key=min):
            entries = sorted(b for b in comp if b == 0 or any(p not in comp for p in self.pred[b]))
            self.loops.append({"blocks": comp, "entries": entries, "parent": parent})
            self._nest(comp, cut | set(entries), len(self.loops) - 1)

    def children(self, k):
        return [i for i, l in enumerate(self.loops) if l["parent"] == k]

    def top_level(self):
        return self.children(None)

    def weights(self, trips, headers=None):
        """block -> product of the trip counts of the loops around it.  A loop whose exit test sits in the middle (the blocks
        behind the test run one time fewer) counts trip - 1 for the blocks reached from the exiting block's in-loop successor
        before the loop's header comes round again.  `headers`: loop index -> header block, for loops with several entries."""
        w = [1] * len(self.blocks)
        for k, l in enumerate(self.loops):
            body, t = l["blocks"], trips[k]
            head = (headers or {}).get(k, l["entries"][0] if len(l["entries"]) == 1 else None)
            assert head is not None, "loop with several entries and no header given"
            exiting = [b for b in body if any(s not in body for s in self.succ[b])]
            late = set()
            if len(exiting) == 1:
                stack = [s_ for s_ in self.succ[exiting[0]] if s_ in body and s_ != head]
                while stack:
                    x = stack.pop()
                    if x in late or x == head:
                        continue
                    late.add(x)
                    stack.extend(y for y in self.succ[x] if y in body)
            for b in body:
                w[b] *= (t - 1) if b in late else t
        return w

    def count(self, w, blocks=None):
        valu = mad = 0
        for b, (lo, hi) in enumerate(self.blocks):
            if blocks is not None and b not in blocks:
                continue
            for i in range(lo, hi):
                op = self.ins[i][1]
                if op.startswith("v_"):
                    valu += w[b]
                    mad += w[b] if op.startswith("v_mad_u64_u32") else 0
        return valu, mad

    def valu_in(self, body):
        return sum(1 for b in body for i in range(*self.blocks[b]) if self.ins[i][1].startswith("v_"))


def general(lib, gt_windows=None):
    if gt_windows is None:
        gt_windows = generator_windows(lib)
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi0EE"))
    top = g.top_level()
    assert len(top) == 4, ("unexpected loop structure of k_verify_fast<ECDSA>", [g.loops[k]["entries"] for k in top])
    inner = g.children(top[2])
    assert len(inner) == 2 and not g.children(top[0]) and not g.children(top[1]) and not g.children(top[3]), ("unexpected inner loops", inner)
    trips = {top[0]: 7, top[1]: 7, top[2]: 32, top[3]: gt_windows - 1, inner[0]: 4, inner[1]: 2}   # (the last generator addition stands apart)
    assert len(trips) == len(g.loops), "loops without a trip count"
    valu, mad = g.count(g.weights(trips))
    regions = {name: g.valu_in(g.loops[k]["blocks"]) for name, k in (("table_fwd", top[0]), ("table_bwd", top[1]), ("doubling", inner[0]),
                                                                      ("addition", inner[1]), ("generator", top[3]))}
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "valu_per_trip": regions, "instructions": len(g.ins)}


def keyed(lib, mode=4, name="ECDSA_KEYED"):
    """k_verify_fast<ECDSA_KEYED> (mode 4) or <SCHNORR_KEYED> (mode 6): the window ladder over the per-call tables"""
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi%dEE" % mode))
    top = g.top_level()
    assert len(top) == 1, ("unexpected loop structure of k_verify_fast<%s>" % name, [g.loops[k]["entries"] for k in top])
    kids = g.children(top[0])
    assert len(kids) == 2, ("unexpected loops inside the round loop", kids)
    chunk = [k for k in kids if g.children(k)]
    dbl = [k for k in kids if not g.children(k)]
    assert len(chunk) == 1 and len(dbl) == 1, "cannot tell the doubling loop from the chunk loop"
    add = g.children(chunk[0])
    assert len(add) == 1 and not g.children(add[0])
    trips = {top[0]: 4, dbl[0]: 4, chunk[0]: 8, add[0]: 2}
    assert len(trips) == len(g.loops), "loops without a trip count"
    # a ROUND starts where the chunk loop is entered from: the block in front of the chunk loop's header
    ch = g.loops[chunk[0]]
    round_head = [p for e in ch["entries"] for p in g.pred[e] if p not in ch["blocks"]]
    assert len(set(round_head)) == 1, ("round header not found", round_head)
    w = g.weights(trips, headers={top[0]: round_head[0]})
    # the doubling loop runs between rounds only: 3 x 4
    assert {w[b] for b in g.loops[dbl[0]]["blocks"]} == {12} and {w[b] for b in g.loops[add[0]]["blocks"]} == {64}, "trip weights are not the source's"
    valu, mad = g.count(w)
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad,
            "valu_per_trip": {"doubling": g.valu_in(g.loops[dbl[0]]["blocks"]), "addition": g.valu_in(g.loops[add[0]]["blocks"])},
            "instructions": len(g.ins)}


def comb(lib, mode=16, name="ECDSA_COMB"):
    """k_verify_fast<ECDSA_COMB> (mode 16) or <SCHNORR_COMB> (mode 17): the round loop (19) with no loop inside - a round is one
    COLUMN (the two entries of the round added to each other and their sum to the accumulator), the exit test, and the
    doubling behind it, which so runs 18 times.  valu_per_trip["addition"] stays the cost per point addition of the 38: HALF a
    column (the column's few instructions of digit extraction included); valu_per_trip["column"] is the whole of it."""
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi%dEE" % mode))
    top = g.top_level()
    assert len(top) == 1, ("unexpected loop structure of k_verify_fast<%s>" % name, [g.loops[k]["entries"] for k in top])
    assert not g.children(top[0]), ("unexpected loops inside the round loop", g.children(top[0]))
    rnd, head = g.loops[top[0]]["blocks"], g.loops[top[0]]["entries"]
    assert len(head) == 1, ("round loop with several entries", head)
    # The round leaves the loop behind its column (j == 0) and runs the doubling otherwise: the doubling's blocks are those
    # the way from the loop's header out of the loop can do without, the column's those it cannot.  (Where the exit stands
    # does not matter: the compiler has put it in a block of its own that the column and the doubling both run into.)
    def leaves_without(skip):
        seen, stack = set(), [head[0]]
        while stack:
            x = stack.pop()
            if x in seen or x == skip:
                continue
            seen.add(x)
            if any(s_ not in rnd for s_ in g.succ[x]):
                return True
            stack.extend(y for y in g.succ[x] if y in rnd)
        return False
    dbl = {b for b in rnd if b != head[0] and leaves_without(b)}
    col = rnd - dbl
    assert dbl and not any(s_ in dbl for s_ in g.succ[head[0]] if g.valu_in({s_}) == 0), "no doubling behind the column"
    w = [1] * len(g.blocks)
    for b in col:
        w[b] = 19
    for b in dbl:
        w[b] = 18
    # 19 columns of two additions each and 18 doublings
    column = g.valu_in(col)
    assert 800 < g.valu_in(dbl) < 1100 and 2400 < column < 3400, "the column and the doubling are not where they were looked for"
    valu, mad = g.count(w)
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad,
            "valu_per_trip": {"doubling": g.valu_in(dbl), "addition": column // 2, "column": column}, "instructions": len(g.ins)}


def comb_nolead(lib, schnorr=False):
    """k_verify_comb<false> (ECDSA) or <true> (BIP-340), comb_ladder.hip: the comb ladder without the lead point.  The first
    round is peeled (one pair sum, straight-line code in front of the loop); the round loop runs 18 times with no loop inside
    and no exit in its middle - the doubling, then the column - so every block of it weighs 18.  No branch stands between
    the doubling and the column (the compiler interleaves them): valu_per_trip["round"] is the whole trip, ["column"] what is
    left of it after the doubling of k_verify_fast<.._COMB> of the same library (the same inlined function), ["addition"]
    half of that, as comb() reports it."""
    g = Cfg(disassemble(lib, "_Z13k_verify_combILb%dEE" % (1 if schnorr else 0)))
    name = "k_verify_comb<%s>" % ("true" if schnorr else "false")
    top = g.top_level()
    assert len(top) == 1, ("unexpected loop structure of " + name, [g.loops[k]["entries"] for k in top])
    assert not g.children(top[0]), ("unexpected loops inside the round loop", g.children(top[0]))
    rnd = g.loops[top[0]]["blocks"]
    w = g.weights({top[0]: 18})
    assert {w[b] for b in rnd} == {18}, ("trip weights of the round loop are not 18 / 18", sorted({w[b] for b in rnd}))
    trip = g.valu_in(rnd)
    dbl = comb(lib, 17 if schnorr else 16)["valu_per_trip"]["doubling"]
    assert 3200 < trip < 4500, "the round (doubling and column) is not where it was looked for"
    valu, mad = g.count(w)
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad,
            "valu_per_trip": {"round": trip, "doubling": dbl, "column": trip - dbl, "addition": (trip - dbl) // 2},
            "loop_trips": {"column": 18, "doubling": 18}, "instructions": len(g.ins)}


def keyset(lib):
    """k_verify_fast<ECDSA_KEYSET>: the ladder over a key set's 32-chunk tables - one chunk loop (32) around the addition loop (2)"""
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi8EE"))
    top = g.top_level()
    assert len(top) == 1, ("unexpected loop structure of k_verify_fast<ECDSA_KEYSET>", [g.loops[k]["entries"] for k in top])
    add = g.children(top[0])
    assert len(add) == 1 and not g.children(add[0])
    trips = {top[0]: 32, add[0]: 2}
    assert len(trips) == len(g.loops), "loops without a trip count"
    valu, mad = g.count(g.weights(trips))
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "valu_per_trip": {"addition": g.valu_in(g.loops[add[0]]["blocks"])},
            "instructions": len(g.ins)}


def keyset_joint(lib):
    """k_verify_fast<ECDSA_KEYSET_JOINT>: one loop over the 32 digit positions, one table addition each"""
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi9EE"))
    top = g.top_level()
    assert len(top) == 1 and not g.children(top[0]), ("unexpected loop structure of k_verify_fast<ECDSA_KEYSET_JOINT>", [g.loops[k]["entries"] for k in top])
    valu, mad = g.count(g.weights({top[0]: 32}))
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "valu_per_trip": {"addition": g.valu_in(g.loops[top[0]]["blocks"])},
            "instructions": len(g.ins)}


def keyset_joint_wide(lib, w):
    """k_verify_fast<ECDSA_KEYSET_JOINT5 / JOINT6>: one loop over the 26 / 22 digit positions, one table addition each"""
    g = Cfg(disassemble(lib, "_Z13k_verify_fastILi%dEE" % (10 if w == 5 else 11)))
    top = g.top_level()
    assert len(top) == 1 and not g.children(top[0]), ("unexpected loop structure of the wide joint ladder", [g.loops[k]["entries"] for k in top])
    valu, mad = g.count(g.weights({top[0]: (128 + w - 1) // w}))
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "valu_per_trip": {"addition": g.valu_in(g.loops[top[0]]["blocks"])},
            "instructions": len(g.ins)}


def _flat_weights(g, trips):
    """block -> product of the trip counts of the loops around it, every block of a loop alike (the wave-per-signature
    kernels' loops are entered in the middle - a prefetch stands in front of them - and leave at their end)"""
    assert len(trips) == len(g.loops), "loops without a trip count"
    w = [1] * len(g.blocks)
    for k, l in enumerate(g.loops):
        for b in l["blocks"]:
            w[b] *= trips[k]
    return w


def _reach(edges, seed):
    """the blocks of `seed` and everything that follows them along `edges` (g.succ: after them, g.pred: before them)"""
    seen, stack = set(seed), list(seed)
    while stack:
        for y in edges[stack.pop()]:
            if y not in seen:
                seen.add(y)
                stack.append(y)
    return seen


def _dominators(g):
    """block -> the set of blocks on every path from the entry to it (itself included); blocks the entry does not reach
    (padding behind the end) keep the full set"""
    nb = len(g.blocks)
    dom = [set(range(nb)) for _ in range(nb)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for b in range(1, nb):
            if g.pred[b]:
                new = set.intersection(*(dom[q] for q in g.pred[b])) | {b}
                if new != dom[b]:
                    dom[b], changed = new, True
    return dom


def _mads_in(g, body):
    return sum(1 for b in body for i in range(*g.blocks[b]) if g.ins[i][1].startswith("v_mad_u64_u32"))


SQRT_CHAIN_TRIPS = [3, 3, 2, 11, 22, 44, 88, 44, 3, 23, 6, 2]      # fer_sqrt_chain's squaring runs (small_call.hip), in order


def row_general(lib, gt_windows=None):
    """k_verify_row, a wave per signature: the key's table (the loop's addition runs 7 times), 32 windows of 4 doublings and two
    additions, gt_windows generator additions.  The straight-line code of the block's preparation wave is in the sum (as it is
    in row_keyset's: the same function)."""
    if gt_windows is None:
        gt_windows = generator_windows(lib)
    g = Cfg(disassemble(lib, "_Z12k_verify_rowj"))
    top = g.top_level()
    assert len(top) == 3, ("unexpected loop structure of k_verify_row", [g.loops[k]["entries"] for k in top])
    dbl = g.children(top[1])
    assert not g.children(top[0]) and len(dbl) == 1 and not g.children(dbl[0]) and not g.children(top[2]), "unexpected inner loops"
    trips = {top[0]: 7, top[1]: 32, dbl[0]: 4, top[2]: gt_windows}
    valu, mad = g.count(_flat_weights(g, trips))
    return {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad,
            "valu_per_trip": {"table": g.valu_in(g.loops[top[0]]["blocks"]), "window": g.valu_in(g.loops[top[1]]["blocks"]),
                              "doubling": g.valu_in(g.loops[dbl[0]]["blocks"]), "generator": g.valu_in(g.loops[top[2]]["blocks"])},
            "instructions": len(g.ins)}


def row_keyset(lib, schnorr=False, gt_windows=None):
    """k_verify_row_keyset / k_schnorr_row_keyset, a wave per signature over a key set's 32-chunk table: one loop over the 32
    chunks with two additions on the key's isomorphic curve each (64 key additions), then gt_windows generator additions.
    BIP-340: the squaring runs of the square-root chain belong to the block's LIFTING wave, not to a signature wave; they
    are counted apart (valu_lift_wave: that wave's chain, for the block's four signatures at once)."""
    if gt_windows is None:
        gt_windows = generator_windows(lib)
    name = "k_schnorr_row_keyset" if schnorr else "k_verify_row_keyset"
    g = Cfg(disassemble(lib, "_Z20k_schnorr_row_keyset" if schnorr else "_Z19k_verify_row_keyset"))
    top = g.top_level()
    assert len(top) == (14 if schnorr else 2) and not any(g.children(k) for k in top), ("unexpected loop structure of " + name, [g.loops[k]["entries"] for k in top])
    chunk, gen, sq = top[0], top[1], top[2:]
    cb, gb = g.loops[chunk]["blocks"], g.loops[gen]["blocks"]
    # two additions with five products each per chunk (one of them a sum of two), one addition of four per window
    assert _mads_in(g, cb) > 2 * _mads_in(g, gb) and all(len(g.loops[k]["blocks"]) == 1 and _mads_in(g, g.loops[k]["blocks"]) == 15 for k in sq), \
        "cannot tell the loops of %s apart" % name
    trips = {chunk: 32, gen: gt_windows}
    trips.update({k: 0 for k in sq})
    valu, mad = g.count(_flat_weights(g, trips))
    out = {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "key_additions": 64, "generator_additions": gt_windows,
           "valu_per_trip": {"chunk": g.valu_in(cb), "generator": g.valu_in(gb)}, "instructions": len(g.ins)}
    if schnorr:
        out["valu_lift_wave"] = sum(t * g.valu_in(g.loops[k]["blocks"]) for t, k in zip(SQRT_CHAIN_TRIPS, sq))
    return out


def row_comb(lib, schnorr=False, gt_windows=None):
    """k_verify_row_comb / k_schnorr_row_comb, a wave per signature over a key set's COMB table: column 18 - a conversion and
    one addition - is straight-line code in front of the round loop, which runs 18 times with no loop inside (a doubling, the
    conversion of the column's two entries, two additions: every block of it weighs 18), then gt_windows generator
    additions.  BIP-340: the lifting wave's squaring runs are counted apart, as row_keyset() does.
    These kernels call nothing (they own no private segment), so the PREPARATION wave's code is in their text where the
    siblings call it.  It belongs to no signature wave and is counted apart, as the lifting wave's runs are: that wave's
    blocks are those on a path through its one loop - the scalar inversion's 20 division-step batches with the step loop
    inside (ECDSA), the message blocks of the challenge hash (BIP-340) - that no path joins with the round loop
    (valu_prep_wave: its straight-line code, the scalar products and the hash's first block; valu_prep_loop: the loop, per
    trip).  What the siblings' preparation wave keeps in the kernel's text (loads, argument set-up, the split) stays in
    their sum."""
    if gt_windows is None:
        gt_windows = generator_windows(lib)
    name = "k_schnorr_row_comb" if schnorr else "k_verify_row_comb"
    g = Cfg(disassemble(lib, "_Z18k_schnorr_row_comb" if schnorr else "_Z17k_verify_row_comb"))
    top = g.top_level()
    assert len(top) == (15 if schnorr else 3) and not any(g.children(k) for k in top[:-1]), ("unexpected loop structure of " + name, [g.loops[k]["entries"] for k in top])
    rnd, gen, sq, prep = top[0], top[1], top[2:-1], top[-1]
    rb, gb, pb = g.loops[rnd]["blocks"], g.loops[gen]["blocks"], g.loops[prep]["blocks"]
    # a round is a doubling, a conversion and two additions (2 + 1 + 2 x 3 layers), a window one addition; the preparation's
    # loop holds no field product at all
    assert _mads_in(g, rb) > 2 * _mads_in(g, gb) and all(len(g.loops[k]["blocks"]) == 1 and _mads_in(g, g.loops[k]["blocks"]) == 15 for k in sq) and \
        _mads_in(g, pb) < 15, "cannot tell the loops of %s apart" % name
    trips = {k: 0 for k in range(len(g.loops))}                     # (the preparation's loop and what is inside it)
    assert all(k in top or set(g.loops[k]["blocks"]) <= set(pb) for k in trips), "a loop inside another than the preparation's"
    trips.update({rnd: 18, gen: gt_windows})
    w = _flat_weights(g, trips)
    assert {w[b] for b in rb} == {18}, ("trip weights of the round loop are not 18", sorted({w[b] for b in rb}))

    # The wave's branch is divergent to the compiler, so its region stands in line with the others' (entered with an empty
    # mask by them): the blocks dominated by the outermost dominator of its loop from which no round loop can follow.
    dom = _dominators(g)
    before_rounds = _reach(g.pred, rb)
    head = g.loops[prep]["entries"][0]
    guards = [d for d in range(len(g.blocks)) if d in dom[head] and d not in before_rounds]
    assert guards, "no block of %s dominates the preparation wave's loop alone" % name
    guard = [d for d in guards if all(d in dom[x] for x in guards)][0]
    prep_wave = {b for b in range(len(g.blocks)) if guard in dom[b]}
    assert set(pb) <= prep_wave and not prep_wave & (set(rb) | set(gb) | set().union(*(g.loops[k]["blocks"] for k in sq), set())), \
        "the preparation wave of %s is not apart from the other waves" % name
    for b in prep_wave:
        w[b] = 0
    valu, mad = g.count(w)
    out = {"valu_instr_static": valu, "mad_u64_u32_per_verify": mad, "key_additions": 37, "key_doublings": 18, "generator_additions": gt_windows,
           "valu_per_trip": {"round": g.valu_in(rb), "generator": g.valu_in(gb)}, "loop_trips": {"round": 18}, "instructions": len(g.ins),
           "valu_prep_wave": g.valu_in(prep_wave - set(pb)), "valu_prep_loop": g.valu_in(pb)}
    if schnorr:
        out["valu_lift_wave"] = sum(t * g.valu_in(g.loops[k]["blocks"]) for t, k in zip(SQRT_CHAIN_TRIPS, sq))
    return out


def generator_windows(lib):
    """ceil(256 / window bits) of THIS library (s2k_generator_window_bits: a host function, no GPU needed)"""
    import ctypes
    bits = int(ctypes.CDLL(os.path.abspath(lib)).s2k_generator_window_bits())
    return (256 + bits - 1) // bits


def static_counts(lib=DEFAULT_LIB, gt_windows=None):
    if gt_windows is None:
        gt_windows = generator_windows(lib)
    out = {"k_verify_fast": general(lib, gt_windows), "k_verify_fast_keyed": keyed(lib), "k_verify_fast_comb": comb(lib),
            "k_verify_fast_keyset": keyset(lib),
            "k_verify_fast_keyset_joint": keyset_joint(lib), "k_verify_fast_keyset_joint5": keyset_joint_wide(lib, 5),
            "k_verify_fast_keyset_joint6": keyset_joint_wide(lib, 6),
            "k_verify_fast_schnorr_keyed": keyed(lib, 6, "SCHNORR_KEYED"), "k_verify_fast_schnorr_comb": comb(lib, 17, "SCHNORR_COMB"),
            "k_verify_row": row_general(lib, gt_windows), "k_verify_row_keyset": row_keyset(lib, False, gt_windows),
            "k_schnorr_row_keyset": row_keyset(lib, True, gt_windows)}
    if has_kernel(lib, "_Z13k_verify_combILb0EE"):      # (a library of before comb_ladder.hip, given for an A/B, has none)
        out["k_verify_comb"] = comb_nolead(lib)
        out["k_verify_comb_schnorr"] = comb_nolead(lib, True)
    if has_kernel(lib, "_Z17k_verify_row_comb"):        # (likewise: a library of before the comb row ladder)
        out["k_verify_row_comb"] = row_comb(lib, False, gt_windows)
        out["k_schnorr_row_comb"] = row_comb(lib, True, gt_windows)
    return out


if __name__ == "__main__":
    print(json.dumps(static_counts(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB), indent=1))
