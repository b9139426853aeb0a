"""Independent checker of the =/X CIGARs (LAMSA_HP_TAG_EQX of the result stream, --eqx of the host program) and of the cs:Z tag
(--cs).  Everything is recomputed with numpy from the packed reference (.pac), the read and the CIGAR in M form; nothing here
shares code with the host program or the device routine (lamsa_amd/csrc/hp_eqx.h).

The =/X form: every M element is replaced, on its own, by its pieces -- the maximal runs of aligned bases that equal the reference
('=', op 7) or differ from it ('X', op 8; a read N differs).  Every other element is copied; pieces never merge across elements."""
import re

import numpy as np

from streamwalk import rebuild, revcomp_codes
from tagcheck import CIG_RE, NT4, ref_codes

OPS = "MIDNSHP=X"
C_M, C_I, C_D, C_S, C_H, C_EQ, C_X = 0, 1, 2, 4, 5, 7, 8


def _pieces(q, t):
    """[(length, differs)] of the maximal runs of q != t."""
    d = (q != t)
    if len(d) == 0:
        return []
    cut = np.flatnonzero(d[1:] != d[:-1]) + 1
    beg = np.concatenate([[0], cut]); end = np.concatenate([cut, [len(d)]])
    return [(int(e - b), bool(d[b])) for b, e in zip(beg, end)]


def to_eqx(words, read_codes, pac, k0):
    """The =/X form of a CIGAR (words len << 4 | op, M form; =/X words pass as they are aligned bases too).  read_codes: the whole read
    as the record aligns it (reverse-complemented for a '-' record; clipped bases, hard-clipped ones too, included).  k0: .pac
    coordinate of the record's first reference base."""
    q = np.asarray(read_codes, np.uint8)
    out, qi, ri = [], 0, 0
    for w in words:
        op, ln = int(w) & 0xf, int(w) >> 4
        if op in (C_M, C_EQ, C_X):
            for n, dif in _pieces(q[qi:qi + ln], ref_codes(pac, k0 + ri, ln)):
                out.append(n << 4 | (C_X if dif else C_EQ))
            qi += ln; ri += ln
        else:
            out.append(int(w))
            if op in (C_I, C_S, C_H):
                qi += ln
            elif op == C_D:
                ri += ln
    return out


def cs_of(words, read_codes, pac, k0):
    """The cs string (minimap2's short form) of a record: `words` in M or =/X form, the rest as for to_eqx."""
    q = np.asarray(read_codes, np.uint8)
    o, qi, ri = [], 0, 0
    for w in words:
        op, ln = int(w) & 0xf, int(w) >> 4
        if op in (C_M, C_EQ, C_X):
            t = ref_codes(pac, k0 + ri, ln)
            j = 0
            for n, dif in _pieces(q[qi:qi + ln], t):
                if dif:
                    o += ["*" + "acgt"[int(t[j + i])] + "acgtn"[int(q[qi + j + i])] for i in range(n)]
                else:
                    o.append(":%d" % n)
                j += n
            qi += ln; ri += ln
        elif op == C_I:
            o.append("+" + "".join("acgtn"[int(c)] for c in q[qi:qi + ln])); qi += ln
        elif op == C_D:
            o.append("-" + "".join("acgt"[int(c)] for c in ref_codes(pac, k0 + ri, ln))); ri += ln
        elif op in (C_S, C_H):
            qi += ln
    return "".join(o)


# ---- the result stream (include/lamsa_hp.h), without mismatch lists
def stream_to_eqx(s, read, pac, seq_off):
    """A read's flag-off stream with every record's cigar_n and CIGAR words replaced by the =/X form."""
    read = np.asarray(read, np.uint8)
    rc = revcomp_codes(read)

    def eqx(r):
        e = to_eqx(r.cig, read if r.nstrand == 1 else rc, pac, r.k0(seq_off))
        return r.hdr[:6] + [len(e)] + e
    return rebuild(s, eqx)


# ---- SAM text
def words_of(cigar):
    return [int(n) << 4 | OPS.index(op) for n, op in CIG_RE.findall(cigar)]


def text_of(words):
    return "".join("%d%s" % (w >> 4, OPS[w & 0xf]) for w in words)


def collapse_cigar(cigar):
    """=/X -> M, neighbouring M merged."""
    out = []
    for n, op in CIG_RE.findall(cigar):
        op = "M" if op in "=X" else op
        if out and out[-1][1] == op == "M":
            out[-1][0] += int(n)
        else:
            out.append([int(n), op])
    return "".join("%d%s" % (n, op) for n, op in out)


_XA_RE = re.compile(r"([^,;]+,[+-]\d+,)([0-9MIDNSHP=X]+)(,\d+;)")
_SA_RE = re.compile(r"([^,;]+,\d+,[+-],)([0-9MIDNSHP=X]+)(,\d+,\d+;)")


def collapse(text):
    """The SAM text with every CIGAR (field 6, inside XA:Z and SA:Z) back in M form and cs:Z removed."""
    out = []
    for l in text.split("\n"):
        if not l or l.startswith("@"):
            out.append(l)
            continue
        f = l.split("\t")
        if f[5] != "*":
            f[5] = collapse_cigar(f[5])
        g = f[:11]
        for t in f[11:]:
            if t.startswith("cs:Z:"):
                continue
            if t.startswith("XA:Z:"):
                t = "XA:Z:" + _XA_RE.sub(lambda m: m.group(1) + collapse_cigar(m.group(2)) + m.group(3), t[5:])
            elif t.startswith("SA:Z:"):
                t = "SA:Z:" + _SA_RE.sub(lambda m: m.group(1) + collapse_cigar(m.group(2)) + m.group(3), t[5:])
            g.append(t)
        out.append("\t".join(g))
    return "\n".join(out)


def load_reads(path):
    """{name: sequence} of a FASTA / FASTQ file with one-line records."""
    reads, lines = {}, open(path).read().split("\n")
    i = 0
    while i < len(lines):
        l = lines[i]
        if l[:1] == ">":
            reads[l[1:].split()[0]] = lines[i + 1]; i += 2
        elif l[:1] == "@":
            reads[l[1:].split()[0]] = lines[i + 1]; i += 4
        else:
            i += 1
    return reads


def check_sam(text, pac, contig_off, reads, eqx=True, cs=True):
    """Every CIGAR the SAM text prints (field 6, XA:Z, SA:Z) and every cs:Z against the recomputation from `reads` ({name: sequence}) and
    the .pac.  eqx / cs: whether the text was made with --eqx / --cs (False: no =/X anywhere / no cs tag).  Returns a list of problems."""
    bad = []

    def want_cigar(name, chrom, pos, minus, cigar):
        q = NT4[np.frombuffer(reads[name].encode(), np.uint8)]
        q = revcomp_codes(q) if minus else q
        k0 = contig_off[chrom] + pos - 1
        w = words_of(collapse_cigar(cigar))
        return text_of(to_eqx(w, q, pac, k0)) if eqx else text_of(w), cs_of(words_of(cigar), q, pac, k0)

    n_cig = 0
    for l in text.split("\n"):
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        tags = dict((t[:2], t[5:]) for t in f[11:])
        if int(f[1]) & 4:
            if "cs" in tags:
                bad.append((f[0], "cs on an unmapped record"))
            continue
        minus = bool(int(f[1]) & 16)
        wc, wcs = want_cigar(f[0], f[2], int(f[3]), minus, f[5])
        n_cig += 1
        if f[5] != wc:
            bad.append((f[0], "CIGAR %s... != %s..." % (f[5][:60], wc[:60])))
        if cs and tags.get("cs") != wcs:
            bad.append((f[0], "cs %s... != %s..." % (str(tags.get("cs"))[:60], wcs[:60])))
        if not cs and "cs" in tags:
            bad.append((f[0], "cs tag without --cs"))
        tag_list = [t[:2] for t in f[11:]]
        order = [t for t in ("NM", "AS", "XA", "MD", "cs", "SA") if t in tag_list]
        if tag_list != order:
            bad.append((f[0], "tag order %s" % tag_list))
        for m in _XA_RE.finditer(tags.get("XA", "")):
            chrom, sp = m.group(1).rstrip(",").split(",")
            wc, _ = want_cigar(f[0], chrom, int(sp[1:]), sp[0] == "-", m.group(2))
            n_cig += 1
            if m.group(2) != wc:
                bad.append((f[0], "XA CIGAR %s... != %s..." % (m.group(2)[:60], wc[:60])))
        for m in _SA_RE.finditer(tags.get("SA", "")):
            chrom, pos, strand = m.group(1).rstrip(",").split(",")
            wc, _ = want_cigar(f[0], chrom, int(pos), strand == "-", m.group(2))
            n_cig += 1
            if m.group(2) != wc:
                bad.append((f[0], "SA CIGAR %s... != %s..." % (m.group(2)[:60], wc[:60])))
    if n_cig == 0:
        bad.append(("*", "no CIGAR checked"))
    return bad
