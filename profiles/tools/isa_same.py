"""isa_same.py OLD.s NEW.s [OLD_SYMBOL=NEW_SYMBOL ...]: are the kernels of two device-assembly files the same code?
(hipcc -save-temps=obj, flags of isa_checks.sh.)  For every kernel present in both files -- or paired by hand on the
command line where its template parameter list changed -- the body between its label and .Lfunc_end, with comments
and .loc / .file / .ident dropped, the function index of local labels (.LBB<n>_) and the kernel's own name replaced by
fixed tokens, must be byte-identical, and so must the register counts, scratch and LDS size of its metadata entry.
One line per kernel; exit status 1 on any difference.  Counterpart of isa_mix.py; compares text only."""
import re
import sys

KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def kernels(path):
    lines = open(path).read().split('\n')
    meta, cur = {}, None
    for l in lines[lines.index('amdhsa.kernels:') + 1 if 'amdhsa.kernels:' in lines else len(lines):]:
        if l.startswith('  - '):
            cur = {}
        m = re.match(r'^(?:  - |    )(\.\w+):\s+(\S+)$', l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == '.symbol':
                meta[m.group(2)[:-3]] = cur                      # (symbol = name + '.kd')
    out = {}
    for name in meta:
        i = next(x for x, l in enumerate(lines) if l.startswith(name + ':'))
        j = next(x for x in range(i, len(lines)) if lines[x].startswith('.Lfunc_end'))
        body = []
        for l in lines[i + 1:j]:
            l = l.split(';')[0].rstrip()
            if not l.strip() or re.match(r'\s*\.(loc|file|ident)\b', l):
                continue
            body.append(re.sub(r'\.LBB\d+_', '.LBB_', l).replace(name, '<kernel>'))
        out[name] = ('\n'.join(body), tuple(meta[name].get(k) for k in KEYS))
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
pairs = [(n, n) for n in old if n in new] + [tuple(a.split('=')) for a in sys.argv[3:]]
paired_old, paired_new = {a for a, _ in pairs}, {b for _, b in pairs}
bad = 0
for a, b in pairs:
    same_body, same_meta = old[a][0] == new[b][0], old[a][1] == new[b][1]
    bad += not (same_body and same_meta)
    n = old[a][0].count('\n') + 1
    verdict = 'same' if same_body and same_meta else 'DIFFERENT' + ('' if same_body else ' body (%d lines now)' % (new[b][0].count('\n') + 1)) + (
        '' if same_meta else ' metadata %s -> %s' % (old[a][1], new[b][1]))
    print('%-9s %6d lines  vgpr/agpr/sgpr/scratch/lds %s  %s%s' % (verdict.split()[0], n, '/'.join(map(str, old[a][1])), a, '' if a == b else ' = ' + b))
    if verdict != 'same':
        print('          ' + verdict)
for n in old:
    if n not in paired_old:
        print('gone      %s' % n)
for n in new:
    if n not in paired_new:
        print('new       %s' % n)
print('%d kernels compared, %d differ' % (len(pairs), bad))
sys.exit(1 if bad else 0)
