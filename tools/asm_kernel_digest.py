#!/usr/bin/env python3
"""asm_kernel_digest.py a.s b.s -- kernel by kernel: sha256 (first 16 hex digits) of the instruction text of two device assembly files
(`make -C vins-mobile_amd/csrc build/digest/<unit>.s`), comments, directives and the numbering of local labels dropped, with the
instruction counts and the resource figures of the kernel descriptors (VGPRs, SGPRs, LDS and scratch bytes). A translation unit that
gains kernels changes its whole-file digest (`make asm-digest`); this shows that the kernels it already had kept their code."""
import hashlib, re, sys

def kernels(path):
    out, cur, name = {}, None, None
    for l in open(path):
        m = re.match(r'^(_Z\w+):', l)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if l.startswith('.Lfunc_end'):
                out[name] = cur
                cur = None
                continue
            s = l.strip()
            if not s or s.startswith(';') or s.startswith('.'):
                continue
            s = re.sub(r';.*$', '', s).strip()
            s = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', s)
            cur.append(s)
    return out

def meta(path):
    txt = open(path).read()
    res = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, re.S):
        b = m.group(2)
        g = lambda k: (re.search(k + r'\s+(\S+)', b) or [None, '?'])[1]
        res[m.group(1)] = dict(vgpr=g(r'\.amdhsa_next_free_vgpr'), sgpr=g(r'\.amdhsa_next_free_sgpr'), accum=g(r'\.amdhsa_accum_offset'),
                               lds=g(r'\.amdhsa_group_segment_fixed_size'), scratch=g(r'\.amdhsa_private_segment_fixed_size'))
    return res

a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
ma, mb = meta(sys.argv[1]), meta(sys.argv[2])
h = lambda x: hashlib.sha256('\n'.join(x).encode()).hexdigest()[:16]
for k in sorted(set(a) | set(b)):
    ha, hb = (h(a[k]) if k in a else '-'), (h(b[k]) if k in b else '-')
    print('%-5s %s %s %5s %5s  %s\n        %s | %s' % ('same' if ha == hb else ('new' if ha == '-' else 'DIFF'), ha, hb, len(a.get(k, [])), len(b.get(k, [])), k, ma.get(k), mb.get(k)))
