#!/usr/bin/env python3
"""VALU wave-instructions per item of the step programs of a pairing, counted statically: the signature bodies of the ahead-of-time kernels in `hipcc -S --offload-arch=gfx950`
listings (counted as tools/isa_blocks.py counts basic blocks) times how often each program runs each signature (`aot_gen --hist`).

usage: valu_per_pairing.py hist.txt sigs.inc listing.s [listing.s ...]      (hist.txt: output of `noble-bls12-381_amd/aot_gen --hist`; sigs.inc: csrc/aot_sigs.inc of the same tree)

A signature's body is one large basic block of its kernel (rounds unrolled, no branch inside).  The compiler lowers the switch over the signatures to a compare tree, so a body is
found by what it must contain, not by a label: a K_DOT body with p0 rounds and t post-added terms has 196 p0 + 14 t (+ 14 with a bias or a weak reduction) signed multiply-adds and
the reduction's 196 unsigned ones, and four LDS operations per operand slot, term and result; a K_LIN body has no multiply-add and four LDS reads per term.  Signatures of one kernel that agree in all of that (they differ in operand shapes only) are
paired with the candidate blocks in order of their size (more flags, mixed-sign operands: the larger body) -- their counts differ by a few dozen instructions, which is the error of the method.  Loads, stores and the step loop
itself (a few VALU instructions per step, mostly scalar work) are counted from the remaining small blocks as a flat per-step figure of the kernel."""
import re
import sys

K_LOAD, K_LIN, K_STORE, K_LOADW, K_STOREW, K_DOT = 0, 2, 3, 4, 5, 12


def blocks_of(path):
    out = {}; kernel = None; cur = None
    for line in open(path):
        m = re.match(r'^([A-Za-z_.][\w.$]*):', line)
        if m and not line.startswith('\t'):
            name = m.group(1)
            if not name.startswith('.L'):
                kernel = name
            cur = dict(valu=0, madi=0, madu=0, ds=0)
            out.setdefault(kernel, []).append(cur)
            continue
        s = line.strip()
        if cur is None or not s or s.startswith(('.', ';')):
            continue
        op = s.split()[0]
        if op.startswith('v_'):
            cur['valu'] += 1
            if op == 'v_mad_i64_i32': cur['madi'] += 1
            elif op == 'v_mad_u64_u32': cur['madu'] += 1
        elif op.startswith('ds_'):
            cur['ds'] += 1
    return out


def sig_tables(path):
    t = {}; name = None
    for line in open(path):
        m = re.match(r'#define AOT_SIGS_(\w+)\(X\)', line)
        if m:
            name = m.group(1); t[name] = []
        m = re.match(r'\s*X\((\d+), (\d+), (\d+), (0x[0-9a-f]+), (\d+), (0x[0-9a-f]+)u, (0x[0-9a-f]+)u,', line)
        if m and name:
            t[name].append(dict(kind=int(m.group(2)), p0=int(m.group(3)), flags=int(m.group(4), 16), t=int(m.group(5)), sh=(int(m.group(6), 16), int(m.group(7), 16))))
    return t


def body_costs(sigs, blocks):
    """VALU instructions of every signature's body + the flat per-step rest"""
    big = [b for b in blocks if b['valu'] >= 40 and b['ds'] >= 8]
    used = set(); cost = [None] * len(sigs)
    def want(s):
        if s['kind'] == K_DOT:
            # signed multiply-adds: the rounds, one pass per post-added term, one for the bias / weak reduction (with a multiplier the bias is a 32-bit multiply and an add);
            # LDS operations: four per 14-limb load (one or two slots per operand by its shape, vm.h SH_*, one per term) and four for the store
            loads = s['t']
            for r in range(s['p0']):
                shape = (s['sh'][0 if r < 4 else 1] >> (8 * (r & 3))) & 0xff
                loads += 2 + (1 if shape & 3 else 0) + (1 if (shape >> 3) & 3 else 0)
            mult = s['flags'] & 3
            return ('dot', 196 * s['p0'] + 14 * s['t'] + (14 if (s['flags'] & 0x0c) and not mult else 0), 4 * loads + 4)
        if s['kind'] == K_LIN:
            return ('lin', 0, 4 * (s['p0'] + s['t']) + 4)
        return None
    groups = {}
    for i, s in enumerate(sigs):
        w = want(s)
        if w: groups.setdefault(w, []).append(i)
    for (kind, key, ds), ids in sorted(groups.items(), key=lambda kv: (-kv[0][1], -kv[0][2])):
        cand = [j for j, b in enumerate(big) if j not in used and abs(b['ds'] - ds) <= 4 and ((kind == 'dot' and b['madu'] >= 190 and abs(b['madi'] - key) <= 8) or (kind == 'lin' and b['madi'] == 0 and b['madu'] == 0))]
        if len(cand) < len(ids):      # (operands normalised first, merged loads: the LDS count is off -- by the multiply-adds alone)
            cand = [j for j, b in enumerate(big) if j not in used and ((kind == 'dot' and b['madu'] >= 190 and abs(b['madi'] - key) <= 8) or (kind == 'lin' and b['madi'] == 0 and b['madu'] == 0 and abs(b['ds'] - ds) <= 8))]
        cand = sorted(cand, key=lambda j: big[j]['valu'])[:len(ids)]
        ids = sorted(ids, key=lambda i: (sigs[i]['flags'], sum(1 for r in range(8) if ((sigs[i]['sh'][r // 4] >> (8 * (r & 3))) & 3) == 3)))      # more flags, mixed-sign operands: the larger body
        if len(cand) < len(ids):      # bodies the compiler merged (identical code for two signatures): reuse the nearest
            cand += [cand[-1]] * (len(ids) - len(cand)) if cand else []
        for i, j in zip(ids, cand):
            cost[i] = big[j]['valu']; used.add(j)
    rest = sum(b['valu'] for j, b in enumerate(blocks) if b['valu'] < 40)
    return cost, rest


def main():
    hist, sigs_path, listings = sys.argv[1], sys.argv[2], sys.argv[3:]
    tables = sig_tables(sigs_path)
    blocks = {}
    for p in listings:
        blocks.update(blocks_of(p))
    for line in open(hist):
        f = line.split()
        kernel, prog, G, nsteps, counts = f[0], f[1], int(f[2]), int(f[3]), [int(x) for x in f[4:]]
        kb = blocks.get('nbls_aot_' + kernel)
        if kb is None or kernel not in tables:
            continue
        cost, rest = body_costs(tables[kernel], kb)
        total = 0; missing = []
        for i, c in enumerate(counts):
            if not c: continue
            if cost[i] is None:
                if tables[kernel][i]['kind'] in (K_DOT, K_LIN): missing.append(i)
                continue
            total += c * cost[i]
        io_steps = sum(c for i, c in enumerate(counts) if tables[kernel][i]['kind'] not in (K_DOT, K_LIN))
        # loads / stores: 14 limbs moved and converted per lane, about 40 VALU instructions a step (the small blocks of the kernel hold all of them once)
        total += io_steps * 40
        print('%-10s %-10s items/wavefront %d  steps %4d  VALU per wavefront %7d  per item %8.1f%s' % (kernel, prog, G, nsteps, total, total / G, '  UNMATCHED signatures %s' % missing if missing else ''))


if __name__ == '__main__':
    main()
