#!/usr/bin/env python3
"""tools/trav_census.py — static instruction census of the traversal pass of one kernel, from `hipcc -S` output.

    hipcc <the Makefile's flags of the unit> --cuda-device-only -S csrc/hjr_launch_nee.hip -o nee.s
    tools/trav_census.py nee.s 'hjr_render_kernelILi0ELb0ELi1024ELb1ELb0ELi2ELi1ELb0ELb0E'     # a substring of the mangled name
    tools/trav_census.py nee.s --all                                                            # resources of every kernel of the file

A developer tool, not a test.  Instructions are classified by mnemonic prefix only:
    valu    v_*                       branch  s_cbranch_* s_branch s_setpc* s_call* s_endpgm
    wait    s_waitcnt* s_nop s_sleep  salu    every other s_*
    ds      ds_*                      vmem    global_* buffer_* flat_* scratch_*
Loops are the natural loops of the kernel's control-flow graph (basic blocks from labels and branches; a back edge is a branch to a block
that dominates its source), so a latch that the compiler laid out in front of the loop's head is counted.  The three loops the tool
reports are found by what they hold:
    node step       the innermost loop with the slab test's v_max3_f32 / v_min3_f32
    triangle loop   the innermost loop with the exact division of ray_tri (v_div_fmas_f32)
    pass body       the innermost loop that holds both
For the node step and the triangle loop it also prints the cheapest trip from the loop's head round to it again and, with --blocks, the
basic blocks in layout order, so that the cost of one path (every lane rejected at `u`, no lane hit, ...) can be added up.
For the whole kernel: VGPRs, AGPRs, SGPRs, spills and scratch from the code object's metadata."""
import argparse
import heapq
import re
import sys

CLASSES = ("valu", "salu", "branch", "ds", "vmem", "wait")


def classify(mn):
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_call", "s_endpgm")):
        return "branch"
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "ds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return None


def kernels_of(text):
    """{mangled name: [(label or None, mnemonic, operands)]} for every function of the file, and the metadata block."""
    out, cur, name = {}, None, None
    for line in text.splitlines():
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            lab = m.group(1)
            if not lab.startswith(".L"):
                name, cur = lab, []
                out[name] = cur
            elif cur is not None:
                cur.append((lab, None, None))
            continue
        t = s.strip()
        if t.startswith("."):
            if t.startswith(".Lfunc_end") or t.startswith(".end_amdhsa_kernel"):
                cur = None
            continue
        if cur is not None:
            parts = t.split(None, 1)
            cur.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def metadata_of(text):
    """{mangled name: {key: int}} from the amdhsa.kernels YAML"""
    res, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\s+-?\s*\.(\w+):\s+(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'\"")
        if k == "agpr_count" and line.lstrip().startswith("-"):
            cur = {}
        if cur is None:
            continue
        if k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            cur[k] = int(v)
        elif k == "name":
            res[v] = cur
    return res


def count(ins):
    c = dict.fromkeys(CLASSES, 0)
    for lab, mn, _ in ins:
        if mn:
            k = classify(mn)
            if k:
                c[k] += 1
    return c


def fmt(c):
    return "  ".join("%s %4d" % (k, c[k]) for k in CLASSES) + "   salu+branch %4d" % (c["salu"] + c["branch"])


def blocks_of(ins):
    """basic blocks of a kernel in layout order: [label, [instructions], [branch target labels], falls through]"""
    blocks, cur, lab = [], [], "(entry)"
    for l, mn, ops in ins:
        if l:
            if cur or lab.startswith(".L") or not blocks:
                blocks.append([lab, cur, [], True])
            lab, cur = l, []
            continue
        cur.append((None, mn, ops))
        if classify(mn) == "branch":
            blocks.append([lab, cur, [ops.strip().split(",")[-1].strip()], not mn.startswith(("s_branch", "s_setpc", "s_endpgm"))])
            lab, cur = "(after %s)" % lab.replace("(after ", "").rstrip(")"), []
    if cur:
        blocks.append([lab, cur, [], False])
    return blocks


def natural_loops(blocks):
    """{header block: set of blocks} from the back edges of the control-flow graph (an edge to a block that dominates its source)"""
    n = len(blocks)
    idx = {}
    for i, bl in enumerate(blocks):
        if bl[0].startswith(".L"):
            idx[bl[0]] = i
    succ = [[idx[t] for t in bl[2] if t in idx] + ([i + 1] if bl[3] and i + 1 < n else []) for i, bl in enumerate(blocks)]
    pred = [[] for _ in range(n)]
    for u in range(n):
        for v in succ[u]:
            pred[v].append(u)
    full = (1 << n) - 1
    dom = [full] * n
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for v in range(1, n):
            d = full
            for u in pred[v]:
                d &= dom[u]
            d = (d | (1 << v)) if pred[v] else (1 << v)
            if d != dom[v]:
                dom[v], changed = d, True
    loops = {}
    for u in range(n):
        for h in succ[u]:
            if dom[u] >> h & 1:
                body, work = loops.setdefault(h, {h}), [u]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(pred[x])
    return loops, succ


def cheapest_trip(blocks, succ, head, body):
    """fewest instructions from the loop's head round to it again, inside the loop: (labels, census)"""
    cost = {u: sum(1 for _, mn, _ in blocks[u][1] if classify(mn)) for u in body}
    dist, prev, heap, closing = {head: cost[head]}, {}, [(cost[head], head)], None
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for v in succ[u]:
            if v == head:
                if closing is None or d < closing[0]:
                    closing = (d, u)
            elif v in body and d + cost[v] < dist.get(v, 1 << 30):
                dist[v], prev[v] = d + cost[v], u
                heapq.heappush(heap, (d + cost[v], v))
    if closing is None:
        return None
    path, u = [closing[1]], closing[1]
    while u != head:
        u = prev[u]
        path.append(u)
    path.reverse()
    return [blocks[u][0] for u in path], count([x for u in path for x in blocks[u][1]])


def report(name, ins, meta, list_blocks):
    print("kernel %s" % name)
    if meta:
        print("  vgpr %d  agpr %d  sgpr %d  vgpr spills %d  sgpr spills %d  scratch %d B  lds %d B" % (
            meta.get("vgpr_count", -1), meta.get("agpr_count", 0), meta.get("sgpr_count", -1), meta.get("vgpr_spill_count", 0),
            meta.get("sgpr_spill_count", 0), meta.get("private_segment_fixed_size", 0), meta.get("group_segment_fixed_size", 0)))
    print("  whole kernel   %s" % fmt(count(ins)))
    blocks = blocks_of(ins)
    loops, succ = natural_loops(blocks)
    body_ins = {h: [x for u in sorted(b) for x in blocks[u][1]] for h, b in loops.items()}
    node = lambda m: any(x[1].startswith(("v_max3_f32", "v_min3_f32")) for x in m)
    tri = lambda m: any(x[1].startswith("v_div_fmas_f32") for x in m)

    def innermost(pred):
        hs = [h for h in loops if pred(body_ins[h])]
        return min(hs, key=lambda h: len(body_ins[h])) if hs else None
    picks = (("node step", innermost(lambda m: node(m) and not tri(m))), ("triangle loop", innermost(lambda m: tri(m) and not node(m))),
             ("pass body", innermost(lambda m: node(m) and tri(m))))
    for what, h in picks:
        if h is None:
            print("  %-14s not found" % what)
            continue
        print("  %-14s %s   (head %s, %d blocks)" % (what, fmt(count(body_ins[h])), blocks[h][0], len(loops[h])))
        if what == "pass body":
            continue
        trip = cheapest_trip(blocks, succ, h, loops[h])
        if trip:
            print("    cheapest trip  %s   via %s" % (fmt(trip[1]), " ".join(trip[0])))
        if list_blocks:
            for u in sorted(loops[h]):
                lab, body, _, _ = blocks[u]
                last = body[-1] if body else None
                end = ("%s %s" % (last[1], last[2])) if last and classify(last[1]) == "branch" else "falls through"
                print("    %-22s %s   %s" % (lab, fmt(count(body)), end))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="output of hipcc --cuda-device-only -S")
    ap.add_argument("kernel", nargs="*", help="substrings of mangled kernel names")
    ap.add_argument("--all", action="store_true", help="resources of every kernel of the file (one line each)")
    ap.add_argument("--blocks", action="store_true", help="list the basic blocks of the node step and the triangle loop")
    a = ap.parse_args()
    text = open(a.asm).read()
    funcs, meta = kernels_of(text), metadata_of(text)
    if a.all:
        for name in sorted(meta):
            m = meta[name]
            print("%s  vgpr %d  agpr %d  vgpr spills %d  sgpr spills %d  scratch %d B" % (name, m.get("vgpr_count", -1), m.get("agpr_count", 0),
                  m.get("vgpr_spill_count", 0), m.get("sgpr_spill_count", 0), m.get("private_segment_fixed_size", 0)))
    rc = 0
    for want in a.kernel:
        hit = [n for n in funcs if want in n and n in meta]
        if len(hit) != 1:
            print("%s: %d kernels match" % (want, len(hit)), file=sys.stderr)
            rc = 1
            continue
        report(hit[0], funcs[hit[0]], meta.get(hit[0]), a.blocks)
    return rc


if __name__ == "__main__":
    sys.exit(main())
