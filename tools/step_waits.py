#!/usr/bin/env python3
"""Where a walk's step waits: the memory issue groups and the s_waitcnt of each step loop, in layout order.

tools/stream_budget.py counts a step's instructions; a wave's time is those plus exposed waits, and a
wait does not show in a count: one s_waitcnt placed before the triangle loads instead of after them costs a memory
latency per step. This script lists, from the same assembly (line tables required):

    ISA_FLAGS=-gline-tables-only tools/isa_one.sh "4,false,false,true,4,false,true,2,true,true,2,true"
    tools/step_waits.py [--asm /tmp/isa/one.s] [--kernel SUBSTR]

for every step loop of the instantiation -- the source lines between `<step:NAME>` and `</step>` comments: the pool's
(rt_shpool.hpp shadow_pool), the closest walk's and the shadow walk's (rt_kernels.hpp) --
  * the VMEM issue groups (runs of loads or stores from one source line) and every s_waitcnt that names vmcnt or
    lgkmcnt, with the source line each was compiled from and, for inlined code, the step's own line that called it;
  * every scalar load (s_load*, s_buffer_load*) on the step's lines;
and the scalar loads per part (stream_budget's line-to-part map). check() turns the listing into the three facts
tests/test_walk_step_isa.py asserts.

A step's instructions are found by their inlined-at chain (the comment clang writes after each .loc): an instruction
belongs to a step loop when some frame of its chain is a line inside the loop's marks. "Between the next-node loads and
a triangle-record load group" is decided on the control-flow graph of the loop's basic blocks (labels and branches in
layout order, edges that leave the loop or go back to its head not followed), not on layout order: the packed path's
block lies between the node loads and the sequential loop in the file but on no path from one to the other that skips
its own loads.
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_budget as sb  # noqa: E402

NODE_FUNCS = ("wload_at", "wload")
TRI_FUNCS = ("tri_load", "hit_triangle", "hit_triangle_at", "hit_tri", "hit_triangle_v")
STEP_PARTS = ("stack", "node test", "triangle tests")
LOC_RE = re.compile(r"([\w.+-]+\.(?:hpp|hip|h)):(\d+):\d+")


def line_info(path):
    """line -> (function, step loop name or None) of one source file"""
    out, fn, step = {}, None, None
    for i, l in enumerate(open(path), 1):
        m = sb.FUNC_RE.match(l)
        if m and not l.rstrip().endswith(";"):
            fn = m.group(1)
        mm = re.search(r"<step:([\w -]+)>", l)
        if mm:
            step = mm.group(1)
        out[i] = (fn, step)
        if "</step>" in l:
            step = None
    return out


class Ins:
    __slots__ = ("pos", "text", "op", "chain", "block")

    def __init__(self, pos, text, chain, block):
        self.pos, self.text, self.op, self.chain, self.block = pos, text, text.split()[0], chain, block


def parse(asm, want):
    """the kernel's instructions in layout order, each with its inlined-at chain [(file, line), ...] (innermost first)
    and its basic block; the blocks' labels"""
    s = open(asm).read()
    body = name = None
    for m in re.finditer(r"^(_ZN[^\s:]*):", s, re.M):
        if want in m.group(1):
            name = m.group(1)
            body = s[m.start():s.index(".Lfunc_end", m.start())]
            break
    if body is None:
        raise SystemExit(f"no kernel matching {want!r} in {asm}")
    ins, labels, chain, block, seen = [], {}, [], 0, False
    for raw in body.split("\n"):
        l = raw.strip()
        if l.startswith(".loc"):
            seen = True
            c = [(f, int(n)) for f, n in LOC_RE.findall(l.split(";", 1)[1])] if ";" in l else []
            if c and c[0][1] != 0:
                chain = c
            continue
        m = re.match(r"(\.LBB\w+):", l)
        if m:
            block += 1
            labels[m.group(1)] = block
            continue
        if not l or l.startswith((";", ".")) or l.endswith(":"):
            continue
        t = l.split(";")[0].strip()
        if not t:
            continue
        ins.append(Ins(len(ins), t, chain, block))
        if t.startswith(("s_cbranch", "s_branch")):
            block += 1  # (the instruction after a branch starts a block)
    if not seen:
        raise SystemExit(f"{asm} has no .loc lines: compile with ISA_FLAGS=-gline-tables-only tools/isa_one.sh ...")
    return name, ins, labels


class Step:
    """one step loop: its instructions, events and control-flow graph"""

    def __init__(self, name, ins, labels, info):
        self.name = name
        self.info = info
        mine = [i for i in ins if self.frame(i) is not None]
        self.empty = not mine
        if self.empty:
            return
        # the loop in layout: from the first to the last instruction compiled from its lines (a loop's latch blocks
        # may lie above its head; edges back to at or above the next-node loads are not followed, see succ)
        node = [i for i in mine if i.op.startswith("global_load") and self.func(i) in NODE_FUNCS]
        first_of = {}
        for i in ins:
            first_of.setdefault(i.block, i.pos)
        self.node_pos = node[0].pos if node else mine[0].pos
        self.lo, self.hi = mine[0].pos, mine[-1].pos
        self.ins = [i for i in ins if self.lo <= i.pos <= self.hi]
        self.first_of, self.labels = first_of, labels
        self.by_block = {}
        for i in self.ins:
            self.by_block.setdefault(i.block, []).append(i)

    def frame(self, i):
        """the step's own source line an instruction belongs to (the outermost frame of its chain inside the marks)"""
        for f, n in reversed(i.chain):
            if self.info.get(f, {}).get(n, (None, None))[1] == self.name:
                return (f, n)
        return None

    def func(self, i):
        f, n = i.chain[0] if i.chain else ("", 0)
        return self.info.get(f, {}).get(n, (None, None))[0]

    def where(self, i):
        f, n = i.chain[0] if i.chain else ("?", 0)
        fr = self.frame(i)
        return f"{f}:{n}" + (f" <- {fr[0]}:{fr[1]}" if fr and fr != (f, n) else "")

    def kind(self, i):
        if i.op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            if i.op.startswith("global_load") and self.func(i) in NODE_FUNCS:
                return "node loads"
            if i.op.startswith("global_load") and self.func(i) in TRI_FUNCS:
                return "triangle loads"
            return "vmem"
        if i.op == "s_waitcnt" and re.search(r"vmcnt|lgkmcnt", i.text):
            return "wait"
        if i.op.startswith(("s_load", "s_buffer_load")):
            return "smem"
        return None

    def events(self):
        """[(kind, first instruction, count)]: groups of consecutive VMEM from one source line; waits; scalar loads"""
        ev = []
        for i in self.ins:
            k = self.kind(i)
            if k is None:
                continue
            if k != "wait" and k != "smem" and ev and ev[-1][0] == k and ev[-1][1].chain[:1] == i.chain[:1] \
                    and ev[-1][1].block == i.block:
                ev[-1] = (k, ev[-1][1], ev[-1][2] + 1)
            else:
                ev.append((k, i, 1))
        return ev

    def succ(self, block):
        """blocks that follow `block` inside the loop, back edges to at or before the node loads not followed"""
        b = self.by_block[block]
        last, out = b[-1], []
        nxt = [k for k in self.by_block if k > block]
        if last.op.startswith(("s_cbranch", "s_branch")):
            t = self.labels.get(last.text.split()[-1])
            if t in self.by_block and self.first_of[t] > self.node_pos:
                out.append(t)
        if not last.op.startswith("s_branch") and nxt:
            out.append(min(nxt))
        return out

    def forward(self, pos):
        """the loop's instructions reachable from position pos, a path ending at the first triangle-record load it
        meets (which is included)"""
        out, seen = [], set()
        blk = next(i.block for i in self.ins if i.pos >= pos)
        todo = [(blk, pos)]
        while todo:
            blk, frm = todo.pop()
            if frm <= self.first_of[blk]:
                if blk in seen:
                    continue
                seen.add(blk)
            ended = False
            for i in self.by_block[blk]:
                if i.pos < frm:
                    continue
                out.append(i)
                if self.kind(i) == "triangle loads":
                    ended = True
                    break
            if not ended:
                todo += [(s, self.first_of[s]) for s in self.succ(blk)]
        return out

    def waits_before_tris(self):
        """[(wait, triangle group's first load)]: the s_waitcnt naming vmcnt that lie on a path from the next-node loads
        to a triangle-record load group (a path that passes no other such group and stays inside the step)"""
        node = [e for e in self.events() if e[0] == "node loads"]
        if not node:
            return []
        out = []
        for w in self.forward(max(i.pos for i in self.ins if self.kind(i) == "node loads") + 1):
            if self.kind(w) == "wait" and "vmcnt" in w.text:
                out += [(w, h) for h in self.forward(w.pos + 1) if self.kind(h) == "triangle loads"]
        return out

    def drains_before_tris(self):
        """the triangle groups directly preceded, in their block, by an s_waitcnt with vmcnt(0)"""
        out = []
        for k, first, _ in self.events():
            if k != "triangle loads":
                continue
            for i in reversed([j for j in self.by_block[first.block] if j.pos < first.pos]):
                kk = self.kind(i)
                if kk == "wait" and re.search(r"vmcnt\(0\)", i.text):
                    out.append((i, first))
                    break
                if kk in ("vmem", "node loads", "triangle loads") or (kk == "wait" and "vmcnt" in i.text):
                    break
        return out

    def tri_groups(self):
        return [first for k, first, _ in self.events() if k == "triangle loads"]

    def smem(self):
        return [i for i in self.ins if self.kind(i) == "smem" and self.frame(i) is not None]


def analyse(asm, want):
    name, ins, labels = parse(asm, want)
    info = {}
    for f in os.listdir(sb.HIP):
        if f.endswith((".hpp", ".hip")):
            info[f] = line_info(os.path.join(sb.HIP, f))
    names = sorted({st for m in info.values() for _, st in m.values() if st})
    steps = [Step(n, ins, labels, info) for n in names]
    _, counts = sb.price(asm, want)
    return name, [s for s in steps if not s.empty], counts


def check(asm, want, pool="pool"):
    """the facts tests/test_walk_step_isa.py asserts, as lists of offending lines (empty: the fact holds)"""
    name, steps, counts = analyse(asm, want)
    bad = {"smem_parts": [], "smem_step": [], "wait_before_tris": [], "drain_before_tris": [], "tri_paths": 0}
    for p in STEP_PARTS:
        n = counts.get(p, {}).get("smem", 0)
        if n:
            bad["smem_parts"].append(f"{p}: {n} scalar loads")
    for st in steps:
        bad["smem_step"] += [f"{st.name}: {i.text} at {st.where(i)}" for i in st.smem()]
        if st.name == pool:
            bad["wait_before_tris"] = [f"{w.text} at {st.where(w)} before the triangle loads of {st.where(h)}"
                                       for w, h in st.waits_before_tris()]
            bad["drain_before_tris"] = [f"{w.text} at {st.where(w)} directly before the triangle loads of {st.where(h)}"
                                        for w, h in st.drains_before_tris()]
            bad["tri_paths"] = len({st.frame(h) for h in st.tri_groups()})
    return name, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="/tmp/isa/one.s")
    ap.add_argument("--kernel", default="k_persist")
    a = ap.parse_args()
    name, steps, counts = analyse(a.asm, a.kernel)
    print(f"kernel {name}")
    print("scalar loads per part: " + ", ".join(f"{p} {c['smem']}" for p, c in sorted(counts.items()) if c["smem"]))
    for st in steps:
        print(f"\nstep loop <{st.name}>: instructions {st.lo}..{st.hi} of the kernel")
        for k, i, n in st.events():
            what = f"{k} x{n}" if k not in ("wait", "smem") else i.text
            print(f"  {i.pos:6d}  block {i.block:4d}  {what:44s} {st.where(i)}")
    _, bad = check(a.asm, a.kernel)
    print()
    for k, v in bad.items():
        if k == "tri_paths":
            print(f"pool step: {v} triangle paths")
        else:
            print(f"{k}: " + ("none" if not v else ""))
            for l in v:
                print("    " + l)


if __name__ == "__main__":
    main()
