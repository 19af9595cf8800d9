"""Per-loop-depth instruction census of one kernel in a hipcc -S listing (gfx950).

usage: python tools/isa_loops.py avr.s <mangled-kernel-name> [depth]
       python tools/isa_loops.py avr.s [mangled-kernel-name] --memory
Counts VALU / SALU / VMEM / LDS / scratch / branch instructions in the basic blocks the
compiler annotates as belonging to loops of the given depth (default: the deepest).
--memory: the far-memory census of the persistent loop (depth >= 1; default kernel: k_paths'
headline instantiation): global loads, scalar loads, s_waitcnt by the counter they drain to
zero, and atomics that return a value (a wave waits for those before it can go on). A static
before / after for changes to the service round that needs no GPU."""
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
    args = [a for a in sys.argv[1:] if a != '--memory']
    text = open(args[0]).read()
    name = args[1] if len(args) > 1 else HEADLINE
    i = text.index(name + ':')
    j = text.index('.Lfunc_end', i)
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
