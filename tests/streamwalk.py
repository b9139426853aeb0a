"""The one walk over a read's result stream (include/lamsa_hp.h: lamsa_hp_result) that the checkers share: tagcheck, eqxcheck, lalcheck
and pafcheck each say what a record becomes, the index arithmetic is here.  A walk is no definition: what the checkers compute per
record stays with them and shares nothing with the product.

Stream of a read: status, lines of round 1, lines of round 2; per line line_score, tol_score, tol_NM, n_res; per record offset_lo,
offset_hi, chr, nstrand, score, NM, cigar_n, then cigar_n CIGAR words (len << 4 | op) -- with LAMSA_HP_TAG_MISMATCHES followed by n_mm and
n_mm event words; with LAMSA_HP_TAG_SUMMARY no CIGAR words but the eight summary words."""
import numpy as np


def revcomp_codes(read):
    """The reverse complement of a read's base codes (0-3, 4 = N): what a '-' record aligns."""
    read = np.asarray(read, np.uint8)
    return np.where(read[::-1] < 4, 3 - read[::-1], 4).astype(np.uint8)


class Record:
    """hdr: the seven header words; cig: the CIGAR words (None in the summary form); mm: the mismatch list (None without lists); sum: the
    eight summary words (None unless the summary form)."""
    __slots__ = ("hdr", "cig", "mm", "sum")

    def __init__(self, hdr, cig, mm, sum_):
        self.hdr, self.cig, self.mm, self.sum = hdr, cig, mm, sum_

    offset = property(lambda r: (r.hdr[0] & 0xffffffff) | (r.hdr[1] << 32))
    chr = property(lambda r: r.hdr[2])
    nstrand = property(lambda r: r.hdr[3])

    def k0(self, seq_off):
        """.pac coordinate of the record's first reference base; seq_off: .pac offset of each contig"""
        return int(seq_off[self.chr - 1]) + self.offset - 1


def walk(s, lists=False, summary=False):
    """Yields ("head", [status, n_lines_1, n_lines_2]), then per line ("line", its four words) and per record ("rec", Record).  The stream of
    a read that failed (status != 0, or fewer than three words) is one ("head", all its words).  lists / summary: the form of the records.
    Asserts that the stream is consumed exactly."""
    s = [int(w) for w in s]
    if len(s) < 3 or s[0] != 0:
        yield "head", s
        return
    yield "head", s[:3]
    i = 3
    for _ in range(s[1] + s[2]):
        yield "line", s[i:i + 4]
        n_res = s[i + 3]; i += 4
        for _ in range(n_res):
            hdr = s[i:i + 7]; i += 7
            cig = mm = sm = None
            if summary:
                sm = s[i:i + 8]; i += 8
                assert len(sm) == 8, "stream ends inside a record"
            else:
                cig = s[i:i + hdr[6]]; i += hdr[6]
                assert len(cig) == hdr[6], "stream ends inside a record"
                if lists:
                    n_mm = s[i]
                    mm = s[i + 1:i + 1 + n_mm]; i += 1 + n_mm
                    assert len(mm) == n_mm, "stream ends inside a record"
            yield "rec", Record(hdr, cig, mm, sm)
    assert i == len(s), "stream not consumed"


def rebuild(s, per_record, **form):
    """The stream with every record replaced by the words per_record(Record) returns; head and line words pass as they are."""
    out = []
    for kind, x in walk(s, **form):
        out += per_record(x) if kind == "rec" else x
    return out


def records(s, **form):
    return [x for kind, x in walk(s, **form) if kind == "rec"]
