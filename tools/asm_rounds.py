"""Design aid: per kernel of the compiled gfx950 code (`make asm` in csrc/ writes /tmp/sactd3_engine.s), the number of scalar-load
ROUNDS a tile block passes between kernel entry and its operand batch, with the kernel descriptor's
`.amdhsa_user_sgpr_kernarg_preload_length` and `.amdhsa_user_sgpr_count`.

A round is one or more `s_load_*` followed by an `s_waitcnt` that waits for them (`lgkmcnt`): what the wave does next -- a branch,
an address -- needs a value that had to come from memory, a scalar-cache miss into the kernel-argument segment each.  (Two batches
that do not depend on each other still count as two rounds when a wait stands between them.)

The path: the kernel's control-flow graph is walked forward from the entry (backward branches are not followed: no kernel here loops
before its first operand request).  The tile block's path is the one with the fewest rounds (then the fewest instructions) to the
kernel's first matrix instruction: riders (Polyak, finalisation, gather, noise blocks) have none, and although the compiler
structurises their code into the same graph (their exit joins the tile code behind a flag register), a path through them is longer.
The OPERAND BATCH is the longest run of vector loads that starts on that path BEHIND the path's first scalar load -- loads in text
order with no full drain (`vmcnt(0)`), barrier, store or loop edge among them; forward branches inside it are passed, a batch may
have optional parts.  (A vector load in front of the first scalar load can only have its address from the launch header -- k_nt asks
for the ring's control words that way -- and is no operand load: counting up to it would count nothing.)  `rounds` is the largest
count in front of any load of the batch that lies on the path, so a round in the middle of the batch counts too; `first` counts up
to the path's first vector load, whatever it is; `batch_line` is the line of the batch's first load within the function's listing.
`rounds_max` is the LARGEST count over the forward paths from the path's first scalar load to any vector load in front of the first
barrier behind the batch (`rounds_max_line`: that load; `off_path_lines`: the loads there that the cheapest path does not pass): what the optional parts of the operand requests wait for, which the cheapest
path branches around -- a ring-reading group of k_nt computes its rows' addresses there.  It says something only where the role is
decided without a load (with a launch header): otherwise the first scalar load stands at the entry and the paths lead through the
riders.  Kernels without matrix instructions: the path to their longest run of loads.
With a preload length > 0 the walk starts behind the compatibility prologue (the 256-byte block at the entry that loads the same
dwords where the firmware does not preload): that is where the packet processor starts a wave whose header it has preloaded.

    python tools/asm_rounds.py [engine.s] [substring of a mangled name ...]
"""
import re
import sys

VLOAD = ("global_load", "buffer_load", "flat_load", "scratch_load")
VMEM_OTHER = ("global_store", "buffer_store", "global_atomic", "buffer_atomic", "flat_store", "flat_atomic")


def _functions(txt):
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n", txt, re.M):
        name = m.group(1)
        end = txt.find(".Lfunc_end", m.end())
        if end < 0:
            continue
        yield name, txt[m.end():end]


def _descriptor(txt, name):
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, re.S)
    if not m:
        return None
    d = m.group(1)

    def field(key):
        f = re.search(r"\." + key + r"\s+(\d+)", d)
        return int(f.group(1)) if f else 0
    return {"preload_length": field("amdhsa_user_sgpr_kernarg_preload_length"), "user_sgpr_count": field("amdhsa_user_sgpr_count")}


def _rounds(body, skip_prologue):
    lines = [l.strip() for l in body.splitlines()]
    ins, labels, at = [], {}, []
    start = 0
    for ln, l in enumerate(lines):
        if not l or l.startswith(";"):
            continue
        if l.startswith(".p2align\t8") or l.startswith(".p2align 8"):
            if skip_prologue and start == 0:
                start = len(ins)
            continue
        m = re.match(r"^(\.?\w+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if l.startswith("."):
            continue
        ins.append(l.split(";")[0].strip())
        at.append(ln)
    n = len(ins)
    INF = (1 << 30, 0)
    best = [[INF, INF] for _ in range(n + 1)]        # best[i][pending]: (fewest rounds, instructions) of a path that arrives in front of i
    prev = [[None, None] for _ in range(n + 1)]
    best[start][0] = (0, 0)

    def push(j, pend, c, frm):
        if j <= n and best[j][pend] > c:
            best[j][pend] = c
            prev[j][pend] = frm
    for i in range(start, n):
        for pend in (0, 1):
            if best[i][pend] == INF:
                continue
            r, steps = best[i][pend]
            op = ins[i]
            if op.startswith("s_endpgm"):
                continue
            p = pend
            if op.startswith("s_load") or op.startswith("s_buffer_load"):
                p = 1
            elif op.startswith("s_waitcnt") and ("lgkmcnt" in op or re.match(r"s_waitcnt\s+0", op)) and pend:
                r, p = r + 1, 0
            c = (r, steps + 1)
            if op.startswith("s_branch"):
                t = labels.get(op.split()[1])
                if t is not None and t > i:
                    push(t, p, c, (i, pend))
                continue
            if op.startswith("s_cbranch"):
                t = labels.get(op.split()[1])
                if t is not None and t > i:
                    push(t, p, c, (i, pend))
            push(i + 1, p, c, (i, pend))

    def run_len(i):                                   # vector loads requested from i on before anything waits for all of them
        k = 0
        for j in range(i, n):
            op = ins[j]
            if op.startswith(VLOAD):
                k += 1
            elif op.startswith(("s_endpgm", "s_barrier")) or op.startswith(VMEM_OTHER):
                break
            elif op.startswith(("s_branch", "s_cbranch")) and labels.get(op.split()[1], n) <= j:
                break                                 # a loop's back edge
            elif op.startswith("s_waitcnt") and "vmcnt(0)" in op:
                break
        return k
    # the tile block's path: the cheapest one to the kernel's first matrix instruction (riders have none); kernels without MFMAs:
    # to their longest run of vector loads
    reach = lambda i: min(best[i][0], best[i][1])
    goal = next((i for i in range(start, n) if ins[i].startswith("v_mfma") and reach(i) != INF), None)
    if goal is None:
        loads = [i for i in range(start, n) if ins[i].startswith(VLOAD) and reach(i) != INF]
        if not loads:
            return None
        goal = max(loads, key=lambda i: (run_len(i), -reach(i)[0], -i))
    st = (goal, 0 if best[goal][0] <= best[goal][1] else 1)
    path = []
    while st is not None:
        path.append(st)
        st = prev[st[0]][st[1]]
    fwd = list(reversed(path))
    on_path = [(i, pend) for i, pend in fwd if ins[i].startswith(VLOAD)]
    if not on_path:
        return None
    # operand loads: what is requested behind the path's first scalar load.  A vector load in front of it can only have its address from
    # the launch header (k_nt's control words) and says nothing about the rounds the operands wait for
    first_s = next((i for i, _ in fwd if ins[i].startswith(("s_load", "s_buffer_load"))), None)
    operand = [s_ for s_ in on_path if first_s is None or s_[0] > first_s] or on_path
    tgt, _ = max(operand, key=lambda s_: (run_len(s_[0]), -s_[0]))
    # every load of the batch that lies on the path counts: a round in the MIDDLE of the batch is a round in front of its later loads
    k, end = 0, tgt
    for j in range(tgt, n):
        if ins[j].startswith(VLOAD):
            k += 1
            end = j
            if k == run_len(tgt):
                break
    rounds = max(best[i][pend][0] for i, pend in operand if tgt <= i <= end)
    # the LARGEST count over the forward paths from the path's first scalar load to any vector load in front of the first barrier behind
    # the batch: the optional parts of the operand requests that the cheapest path branches around (k_nt: a ring-reading group's rows)
    worst, worst_at, off_path = rounds, tgt, []
    on_min = {i for i, _ in fwd}
    if first_s is not None:
        stop = next((j for j in range(end, n) if ins[j].startswith(("s_barrier", "s_endpgm"))), n)
        base = next(best[i][pend][0] for i, pend in fwd if i == first_s)
        NONE = -1
        far = [[NONE, NONE] for _ in range(stop + 1)]
        far[first_s][0] = base

        def reach_far(j, pend, r):
            if j <= stop and far[j][pend] < r:
                far[j][pend] = r
        for i in range(first_s, stop):
            for pend in (0, 1):
                r = far[i][pend]
                if r == NONE:
                    continue
                op = ins[i]
                if op.startswith(VLOAD) and r > worst:
                    worst, worst_at = r, i
                if op.startswith(VLOAD) and i not in on_min and at[i] not in off_path:
                    off_path.append(at[i])
                p = pend
                if op.startswith("s_load") or op.startswith("s_buffer_load"):
                    p = 1
                elif op.startswith("s_waitcnt") and ("lgkmcnt" in op or re.match(r"s_waitcnt\s+0", op)) and pend:
                    r, p = r + 1, 0
                if op.startswith(("s_branch", "s_cbranch")):
                    t = labels.get(op.split()[1])
                    if t is not None and t > i:
                        reach_far(t, p, r)
                    if op.startswith("s_branch"):
                        continue
                reach_far(i + 1, p, r)
    return {"rounds": rounds, "batch": run_len(tgt), "first": best[on_path[0][0]][on_path[0][1]][0], "batch_line": at[tgt],
            "rounds_max": worst, "rounds_max_line": at[worst_at], "off_path_lines": off_path}


def analyse(txt, want=None):
    """{mangled name: {preload_length, user_sgpr_count, rounds, batch, first, batch_line, rounds_max, rounds_max_line, off_path_lines}} for the kernels of an assembly listing: rounds in front of
    the operand batch, the batch's length, rounds in front of the path's first vector load"""
    out = {}
    for name, body in _functions(txt):
        if want and not any(w in name for w in want):
            continue
        d = _descriptor(txt, name)
        if d is None:
            continue                                  # not a kernel
        r = _rounds(body, d["preload_length"] > 0) or {"rounds": None, "batch": 0, "first": None, "batch_line": None, "rounds_max": None, "rounds_max_line": None, "off_path_lines": []}
        d.update(r)
        out[name] = d
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else "/tmp/sactd3_engine.s"
    res = analyse(open(path).read(), sys.argv[2:])
    print("%-72s %7s %9s %6s %5s %5s %10s" % ("kernel", "preload", "user_sgpr", "rounds", "batch", "first", "rounds_max"))
    for name, d in res.items():
        print("%-72s %7d %9d %6s %5d %5s %10s" % (name[:72], d["preload_length"], d["user_sgpr_count"], d["rounds"], d["batch"], d["first"], d["rounds_max"]))
