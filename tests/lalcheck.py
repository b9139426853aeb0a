"""Independent checker of the left-aligned gaps (LAMSA_HP_TAG_LEFT_ALIGN of the result stream, --left-align of the host program).
The definition of include/lamsa_hp.h is run as it is written there, element by element and base by base, from the packed reference
(.pac), the read and the CIGAR in M form; nothing here shares code with the host program or the device routine
(lamsa_amd/csrc/hp_lalign.h).

    for i = 0 .. n-1, ascending:
        if op[i] in {I, D} and 0 < i < n-1 and op[i-1] == M and op[i+1] == M:
            k = len[i]; q = read position of element i; p = reference position of element i
            while len[i-1] > 1 and ( op[i] == D ? T[p-1] == T[p+k-1] : R[q-1] == R[q+k-1] ):
                len[i-1] -= 1; len[i+1] += 1; p -= 1; q -= 1

Counters (a dict handed in as `stats` is added to): "gaps" = I / D elements seen, "moved" = those that moved, "room" = the movable ones
(moved or not) that stopped only because the M before them ran out (the bases would have let them go on: s < f), "cascade" = those that moved further than the M
before them was long at the start (s > len[i-1] - 1: they used what the gap before them had freed), "cascade_block" = the cascades
whose previous gap lies in another block of 64 elements."""
import re

import numpy as np

from eqxcheck import _SA_RE, _XA_RE, collapse, text_of, words_of
from streamwalk import rebuild, revcomp_codes
from tagcheck import NT4, ref_codes

C_M, C_I, C_D, C_S, C_H = 0, 1, 2, 4, 5
COUNTERS = ("gaps", "moved", "room", "cascade", "cascade_block")


def new_stats():
    return dict((k, 0) for k in COUNTERS)


def left_align(words, read_codes, pac, k0, stats=None):
    """The CIGAR `words` (len << 4 | op, M form) left-aligned.  read_codes: the whole read as the record aligns it (reverse-complemented
    for a '-' record; clipped bases, hard-clipped ones too, included); k0: .pac coordinate of the record's first reference base."""
    op = [int(w) & 0xf for w in words]
    ln = [int(w) >> 4 for w in words]
    orig = list(ln)
    n = len(op)
    R = np.asarray(read_codes, np.uint8).tolist()
    T = ref_codes(pac, k0, sum(l for o, l in zip(op, ln) if o in (C_M, C_D))).tolist()
    q = p = 0
    for i in range(n):
        if op[i] in (C_I, C_D):
            if stats is not None:
                stats["gaps"] += 1
            if 0 < i < n - 1 and op[i - 1] == C_M and op[i + 1] == C_M:
                k, s = ln[i], 0
                X, x = (T, p) if op[i] == C_D else (R, q)
                while ln[i - 1] > 1 and X[x - 1] == X[x + k - 1]:
                    ln[i - 1] -= 1; ln[i + 1] += 1; x -= 1; s += 1
                q -= s; p -= s                                         # the element starts s bases further left on both
                if stats is not None and x >= 1 and X[x - 1] == X[x + k - 1]:      # the bases would let it go on: only the M ran out
                    stats["room"] += 1
                if stats is not None and s > 0:
                    stats["moved"] += 1
                    if s > orig[i - 1] - 1:                            # further than the M before it was long: the gap before it made room
                        stats["cascade"] += 1
                        if (i - 2) // 64 != i // 64:
                            stats["cascade_block"] += 1
        if op[i] in (C_M, C_I, C_S, C_H):
            q += ln[i]
        if op[i] in (C_M, C_D):
            p += ln[i]
    return [l << 4 | o for o, l in zip(op, ln)]


def check_consequences(before, after):
    """The stated consequences of the definition that can be seen on the two CIGARs alone; returns a list of problems."""
    bad = []
    if len(before) != len(after):
        return ["element count"]
    for i, (a, b) in enumerate(zip(before, after)):
        if (a & 0xf) != (b & 0xf):
            bad.append("op of element %d" % i)
        elif (a & 0xf) != C_M and a != b:
            bad.append("length of element %d (not an M)" % i)
        elif (b >> 4) < 1 and (a >> 4) >= 1:
            bad.append("M %d consumed" % i)
    if sum(a >> 4 for a in before if a & 0xf == C_M) != sum(b >> 4 for b in after if b & 0xf == C_M):
        bad.append("aligned bases")
    return bad


# ---- the result stream (include/lamsa_hp.h), without mismatch lists
def stream_left_aligned(s, read, pac, seq_off, stats=None):
    """A read's flag-off stream with the CIGAR words of every record replaced by the left-aligned ones; no other word changes."""
    read = np.asarray(read, np.uint8)
    rc = revcomp_codes(read)
    return rebuild(s, lambda r: r.hdr + left_align(r.cig, read if r.nstrand == 1 else rc, pac, r.k0(seq_off), stats))


# ---- SAM text
def _strip_md(text):
    return re.sub(r"\tMD:Z:[^\t\n]*", "", text)


def _la_line(l, la):
    """One SAM line with its CIGARs (field 6, XA:Z, SA:Z) replaced by la(name, contig, pos, is_minus, cigar); the number replaced."""
    if not l or l.startswith("@"):
        return l, 0
    f = l.split("\t")
    if int(f[1]) & 4:
        return l, 0
    name, n = f[0], 1
    f[5] = la(name, f[2], int(f[3]), bool(int(f[1]) & 16), f[5])
    for j in range(11, len(f)):
        if f[j].startswith("XA:Z:"):
            def xa(m):
                chrom, sp = m.group(1).rstrip(",").split(",")
                return m.group(1) + la(name, chrom, int(sp[1:]), sp[0] == "-", m.group(2)) + m.group(3)
            f[j], k = _XA_RE.subn(xa, f[j][5:]); f[j] = "XA:Z:" + f[j]; n += k
        elif f[j].startswith("SA:Z:"):
            def sa(m):
                chrom, pos, strand = m.group(1).rstrip(",").split(",")
                return m.group(1) + la(name, chrom, int(pos), strand == "-", m.group(2)) + m.group(3)
            f[j], k = _SA_RE.subn(sa, f[j][5:]); f[j] = "SA:Z:" + f[j]; n += k
    return "\t".join(f), n


def replace_cigars(plain_sam, pac, contig_off, reads, stats=None):
    """(plain_sam -- CIGARs in M form -- with every CIGAR replaced by the checker's left-aligned one, the number of CIGARs replaced).
    reads: {name: sequence} of the read file; a '-' record aligns the reverse complement."""
    def la(name, chrom, pos, minus, cigar):
        q = NT4[np.frombuffer(reads[name].encode(), np.uint8)]
        q = revcomp_codes(q) if minus else q
        return text_of(left_align(words_of(cigar), q, pac, contig_off[chrom] + pos - 1, stats))
    out, n = [], 0
    for l in plain_sam.split("\n"):
        w, k = _la_line(l, la)
        out.append(w); n += k
    return "\n".join(out), n


def check_sam(plain_sam, la_sam, pac, contig_off, reads, stats=None):
    """la_sam (made with --left-align) against plain_sam (the same run without it): it must be the plain text with every CIGAR -- field 6,
    inside XA:Z and SA:Z -- replaced by the checker's.  Both texts are compared in M form and without MD:Z / cs:Z (those follow the CIGAR
    and have checkers of their own: tagcheck.check_sam, eqxcheck.check_sam); @PG lines are not compared.  Returns a list of problems."""
    want, n_cig = replace_cigars(_strip_md(collapse(plain_sam)), pac, contig_off, reads, stats)
    a = [l for l in want.split("\n") if not l.startswith("@PG")]
    b = [l for l in _strip_md(collapse(la_sam)).split("\n") if not l.startswith("@PG")]
    if len(a) != len(b):
        return [("*", "%d lines against %d" % (len(b), len(a)))]
    bad = []
    for w, g in zip(a, b):
        if w != g:
            f, h = w.split("\t"), g.split("\t")
            k = [j for j in range(min(len(f), len(h))) if f[j] != h[j]]
            bad.append((f[0], "field %s: %s... != %s..." % (k[:1], (h[k[0]] if k else "")[:80], (f[k[0]] if k else "")[:80])))
    if n_cig == 0:
        bad.append(("*", "no CIGAR checked"))
    return bad
