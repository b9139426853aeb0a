"""An independent checker for LAMSA_HP_TAG_SUMMARY and the PAF writer (--paf / --paf-cg).  It shares no code with the product: the
summary words are computed here from the words of a flag-off result stream, the PAF lines from SAM text alone.

Result stream of a read (include/lamsa_hp.h): status, lines of round 1, lines of round 2; per line line_score, tol_score, tol_NM,
n_res; per record offset_lo, offset_hi, chr, nstrand, score, NM, cigar_n and cigar_n words len << 4 | op.  With the item set the
record is these seven words and q_beg, q_end, ref_span, m_bases, ins_bases, del_bases, ins_runs, del_runs."""
import re

from streamwalk import walk

M, I, D, S, H, EQ, X = 0, 1, 2, 4, 5, 7, 8


def new_stats():
    """What the inputs exercise: '-' records, records clipped on both ends, lines of more than one record (counted on streams only:
    SAM text does not say where a line ends), records of more than 64 CIGAR elements (more than one block of lanes in res_aux),
    records with an I next to a D (two runs), XA lines (counted on SAM text only)."""
    return {"minus": 0, "both_clips": 0, "multi_rec": 0, "long_cigar": 0, "adjacent_id": 0, "xa": 0}


def summary_words(cigar, nstrand, read_len, stats=None):
    """The eight words of a record from its CIGAR words (M form, or =/X: 7 and 8 count as M)."""
    ops = [w & 0xf for w in cigar]
    lens = [w >> 4 for w in cigar]
    m = sum(n for o, n in zip(ops, lens) if o in (M, EQ, X))
    ins = sum(n for o, n in zip(ops, lens) if o == I)
    dele = sum(n for o, n in zip(ops, lens) if o == D)
    lead = lens[0] if ops and ops[0] == S else 0
    trail = lens[-1] if ops and ops[-1] == S else 0
    if nstrand != 1:
        lead, trail = trail, lead
    if stats is not None:
        stats["minus"] += nstrand != 1
        stats["both_clips"] += len(ops) >= 2 and ops[0] == S and ops[-1] == S and lens[0] > 0 and lens[-1] > 0
        stats["long_cigar"] += len(ops) > 64
        stats["adjacent_id"] += any({a, b} == {I, D} for a, b in zip(ops, ops[1:]))
    return [lead + 1, read_len - trail, m + dele, m, ins, dele, ops.count(I), ops.count(D)]


def stream_summaries(words, read_len, para=None, stats=None):
    """The flag-off stream of one read -> the stream LAMSA_HP_TAG_SUMMARY must give.  Asserts the two identities on every record:
    n_mm = NM - ins_bases - del_bases >= 0, and (with para, an object with the scoring fields) the score formula."""
    out = []
    for kind, x in walk(words):
        if kind == "head":
            assert len(x) <= 3
        elif kind == "line" and stats is not None:
            stats["multi_rec"] += x[3] > 1
        if kind != "rec":
            out += x
            continue
        hdr = x.hdr
        s = summary_words(x.cig, hdr[3], read_len, stats)
        q_beg, q_end, ref_span, m, ins, dele, io, do = s
        n_mm = hdr[5] - ins - dele
        assert n_mm >= 0, (hdr, s)
        assert 1 <= q_beg <= q_end <= read_len, (hdr, s)
        if para is not None:
            assert hdr[4] == (m - n_mm) * para.match - n_mm * para.mis - io * para.ins_gapo - ins * para.ins_gape - do * para.del_gapo - dele * para.del_gape, (hdr, s)
        out += hdr + s
    return out


_CIG = re.compile(r"(\d+)([MIDNSHP=X])")


def _paf_cols(name, cigar, strand, contig, contig_len, pos, mapq, nm, stats=None):
    el = [(int(n), o) for n, o in _CIG.findall(cigar)]
    assert "".join("%d%s" % e for e in el) == cigar and el
    read_len = sum(n for n, o in el if o in "MIS=XH")
    m = sum(n for n, o in el if o in "M=X")
    ins = sum(n for n, o in el if o == "I")
    dele = sum(n for n, o in el if o == "D")
    io = sum(1 for n, o in el if o == "I")
    do = sum(1 for n, o in el if o == "D")
    lead = el[0][0] if el[0][1] in "SH" else 0
    trail = el[-1][0] if el[-1][1] in "SH" else 0
    if strand == "-":
        lead, trail = trail, lead
    n_mm = nm - ins - dele
    assert n_mm >= 0
    if stats is not None:
        stats["minus"] += strand == "-"
        stats["both_clips"] += len(el) >= 2 and el[0][1] in "SH" and el[-1][1] in "SH" and el[0][0] > 0 and el[-1][0] > 0
        stats["long_cigar"] += len(el) > 64
        stats["adjacent_id"] += any({a[1], b[1]} == {"I", "D"} for a, b in zip(el, el[1:]))
    den = m + io + do
    de = "%.4f" % ((n_mm + io + do) / den) if den else "0.0000"
    cols = [name, read_len, lead, read_len - trail, strand, contig, contig_len[contig], pos - 1, pos - 1 + m + dele, m - n_mm, m + ins + dele, mapq]
    cg = "".join("%d%s" % e for e in el if e[1] not in "SH")
    return [str(c) for c in cols], de, cg


def sam_to_paf(sam_text, contig_len, cg=False, stats=None):
    """The PAF text the SAM text stands for: a line per mapped record (tp:A:P, NM, AS, de), behind it a line per entry of its XA:Z
    (tp:A:S, NM, de; mapQ 0).  cg: with cg:Z (the CIGAR without its clips) and the record's MD:Z / cs:Z where the SAM line has them.
    Nothing but the SAM text is read: the read length is the CIGAR's (S and H included), the mismatches are NM - I - D."""
    out = []
    for ln in sam_text.split("\n"):
        if not ln or ln.startswith("@"):
            continue
        f = ln.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        tags = {t[:5]: t[5:] for t in f[11:]}
        strand = "-" if flag & 16 else "+"
        cols, de, cgs = _paf_cols(f[0], f[5], strand, f[2], contig_len, int(f[3]), int(f[4]), int(tags["NM:i:"]), stats)
        line = cols + ["tp:A:P", "NM:i:" + tags["NM:i:"], "AS:i:" + tags["AS:i:"], "de:f:" + de]
        if cg:
            line.append("cg:Z:" + cgs)
            for t in ("MD:Z:", "cs:Z:"):
                if t in tags:
                    line.append(t + tags[t])
        out.append("\t".join(line))
        if "XA:Z:" in tags:
            for e in tags["XA:Z:"].split(";"):
                if not e:
                    continue
                chrom, sp, cigar, nm = e.rsplit(",", 3)
                cols, de, cgs = _paf_cols(f[0], cigar, sp[0], chrom, contig_len, int(sp[1:]), 0, int(nm), stats)
                line = cols + ["tp:A:S", "NM:i:" + nm, "de:f:" + de]
                if cg:
                    line.append("cg:Z:" + cgs)
                out.append("\t".join(line))
                if stats is not None:
                    stats["xa"] += 1
    return "".join(l + "\n" for l in out)


def contig_lengths(sam_text):
    """{name: length} of the @SQ lines."""
    d = {}
    for ln in sam_text.split("\n"):
        if ln.startswith("@SQ"):
            f = dict(t.split(":", 1) for t in ln.split("\t")[1:])
            d[f["SN"]] = int(f["LN"])
    return d
