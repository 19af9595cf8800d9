"""Per-loop-depth instruction census of one kernel in a hipcc -S listing (gfx950).

usage: python tools/isa_loops.py avr.s <mangled-kernel-name> [depth]
       python tools/isa_loops.py avr.s [mangled-kernel-name] --memory
       python tools/isa_loops.py avr.s [mangled-kernel-name] --tracking
Counts VALU / SALU / VMEM / LDS / scratch / branch instructions in the basic blocks the
compiler annotates as belonging to loops of the given depth (default: the deepest).
--memory: the far-memory census of the persistent loop (depth >= 1; default kernel: k_paths'
headline instantiation): global loads, scalar loads, s_waitcnt by the counter they drain to
zero, and atomics that return a value (a wave waits for those before it can go on). A static
before / after for changes to the service round that needs no GPU.
--tracking: k_paths' tracking loop. The walk loop is the innermost loop that advances the segment
RNG (it holds PCG32's multiplier as a literal) inside a loop of depth 2, the tracking loop; one
trip of the walk is the walk loop's instruction count. The collision block (exact candidate,
density fetch, callbacks) is what the tracking loop lays out behind the walk loop."""
import re
import sys
from collections import Counter


def blocks(lines):
    cur, depth, out = None, 0, []
    for l in lines:
        m = re.match(r'^(\.LBB\S+|; %bb\.\d+):', l.strip())
        if m or l.startswith('.LBB'):
            if cur is not None:
                out.append((depth, cur))
            cur = []
            d = re.search(r'Depth=(\d+)', l)
            depth = int(d.group(1)) if d else 0
            continue
        if cur is None:
            cur = []
        s = l.strip()
        if not s or s.startswith(';') or s.startswith('.'):
            d = re.search(r'Depth=(\d+)', s)
            if d and not cur:
                depth = int(d.group(1))
            continue
        cur.append(s)
    if cur is not None:
        out.append((depth, cur))
    return out


HEADLINE = "_ZN3avr7k_pathsILb0ELb1ELi3ELi0ELb0ELb0EEEvNS_6ParamsE"


def memory_census(bl, want=1):
    """Counts over the blocks of loop depth >= want: loads, waits and returning atomics."""
    c = Counter()
    for d, ins in bl:
        if d < want:
            continue
        for s in ins:
            op = s.split()[0]
            if op.startswith(('global_load', 'buffer_load', 'flat_load')):
                c['global/buffer loads'] += 1
            elif op.startswith(('s_load', 's_buffer_load')):
                c['scalar loads'] += 1
            elif op.startswith('ds_') and ('read' in op or 'load' in op):
                c['LDS reads'] += 1
            elif op == 's_waitcnt':
                c['s_waitcnt'] += 1
                for cnt in ('vmcnt', 'lgkmcnt'):
                    if cnt + '(0)' in s:
                        c[f's_waitcnt {cnt}(0)'] += 1
            elif op.startswith(('global_atomic', 'buffer_atomic', 'flat_atomic')):
                # gfx950 marks an atomic that returns the old value with sc0 (glc before gfx940)
                c['returning atomics' if re.search(r'\b(sc0|glc)\b', s) else 'atomics without return'] += 1
    return c


PCG_MULT_LO = "0x4c957f2d"


def loop_blocks(lines):
    """Basic blocks in layout order as (loop header or None, depth, [parent headers], instrs)."""
    out = []
    n = len(lines)
    for i, l in enumerate(lines):
        s = l.strip()
        m = re.match(r'^(\.LBB\d+_\d+):', s)
        if not (m or re.match(r'^; %bb\.\d+:', s)):
            if out and s and not s.startswith((';', '.')):
                out[-1][3].append(s)
            continue
        ann, q = l, i + 1
        while q < n and lines[q].strip().startswith(';') and not re.match(r'^; %bb\.\d+:', lines[q].strip()):
            ann += '\n' + lines[q]
            q += 1
        inl = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', ann)
        hdr = re.search(r'Loop Header: Depth=(\d+)', ann)
        if inl:
            head, depth = inl.group(1), int(inl.group(2))
        elif hdr and m:
            head, depth = m.group(1)[2:], int(hdr.group(1))
        else:
            head, depth = None, 0
        out.append((head, depth, [h for h, _ in re.findall(r'Parent Loop (BB\d+_\d+) Depth=(\d+)', ann)], []))
    return out


def tracking_census(lines):
    """(walk loop header, its instruction count, tracking loop header, collision block count)."""
    bl = loop_blocks(lines)
    parent = {h: par[-1] for h, d, par, _ in bl if h and par}
    depth = {h: d for h, d, _, _ in bl if h}
    walks = [h for h, d, _, ins in bl if h and depth[h] >= 3 and depth.get(parent.get(h)) == 2
             and any(PCG_MULT_LO in s for s in ins)]
    if not walks:
        raise SystemExit("no walk loop found (no loop of depth 3 holds PCG32's multiplier)")
    walk = walks[-1]
    track = parent[walk]
    last = max(i for i, b in enumerate(bl) if b[0] == walk)
    trip = sum(len(b[3]) for b in bl if b[0] == walk)
    coll = sum(len(b[3]) for i, b in enumerate(bl) if b[0] == track and i > last)
    return walk, trip, track, coll


def kind(op):
    op = op.split()[0]
    if op.startswith('scratch_'):
        return 'scratch'
    if op.startswith(('global_', 'buffer_', 'flat_')):
        return 'vmem'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('s_cbranch', 's_branch')):
        return 'branch'
    if op.startswith('s_waitcnt') or op.startswith('s_nop'):
        return 'wait/nop'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('v_mov'):
        return 'v_mov'
    if op.startswith('v_') and '_f64' in op:
        return 'valu_f64'
    if op.startswith('v_'):
        return 'valu'
    return 'other'


def main():
    args = [a for a in sys.argv[1:] if a not in ('--memory', '--tracking')]
    text = open(args[0]).read()
    name = args[1] if len(args) > 1 else HEADLINE
    i = text.index(name + ':')
    j = text.index('.Lfunc_end', i)
    if '--tracking' in sys.argv[1:]:
        walk, trip, track, coll = tracking_census(text[i:j].split('\n'))
        print(f"{name}: walk loop {walk}: {trip} instrs per trip; collision block (tracking loop {track} behind the walk): "
              f"{coll} instrs")
        return
    bl = blocks(text[i:j].split('\n'))
    if '--memory' in sys.argv[1:]:
        c = memory_census(bl)
        print(f"{name} depth>=1: " + ", ".join(f"{k} {c[k]}" for k in sorted(c)))
        return
    maxd = max(d for d, _ in bl)
    want = int(args[2]) if len(args) > 2 else maxd
    tot = Counter()
    nb = 0
    for d, ops in bl:
        if d >= want:
            nb += 1
            for op in ops:
                tot[kind(op)] += 1
    allc = Counter(kind(op) for _, ops in bl for op in ops)
    print(f"depth>={want} (max {maxd}): {nb} blocks, {sum(tot.values())} instrs: {dict(tot)}")
    print(f"whole kernel: {sum(allc.values())} instrs: {dict(allc)}")


if __name__ == '__main__':
    main()
