"""Independent checker of the optional SAM tags (--MD, --SA) and of the mismatch lists of the result stream
(lamsa_hp_set_result_tags, LAMSA_HP_TAG_MISMATCHES).  MD is recomputed from the packed reference (.pac) and each
record's POS, CIGAR and SEQ as printed; nothing here shares code with the host program."""
import re

import numpy as np

from streamwalk import rebuild, records, revcomp_codes

MD_RE = re.compile(r"^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$")
NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    NT4[ord(_c)] = NT4[ord(_c.lower())] = _i
CIG_RE = re.compile(r"(\d+)([MIDNSHP=X])")


def load_ref(prefix):
    """(.pac bytes as uint8, {contig name: .pac offset}) of an index prefix (bwa's .ann layout)."""
    pac = np.fromfile(prefix + ".pac", np.uint8)
    lines = open(prefix + ".ann").read().split("\n")
    n = int(lines[0].split()[1])
    off = {}
    for i in range(n):
        name = lines[1 + 2 * i].split()[1]
        off[name] = int(lines[2 + 2 * i].split()[0])
    return pac, off


def ref_codes(pac, k0, n):
    """n reference base codes (0-3) from .pac coordinate k0."""
    k = np.arange(k0, k0 + n, dtype=np.int64)
    return (pac[k >> 2] >> ((~k & 3) << 1).astype(np.uint8)) & 3


def md_nm(pac, k0, cigar, seq):
    """(MD string, NM) of a record at .pac coordinate k0 (its POS) with `cigar` [(len, op)] and SEQ as printed."""
    q = NT4[np.frombuffer(seq.encode(), np.uint8)] if seq != "*" else np.zeros(0, np.uint8)
    qi = ri = 0
    md, run, nm = [], 0, 0
    for ln, op in cigar:
        if op == "M":
            t = ref_codes(pac, k0 + ri, ln)
            diff = np.nonzero(q[qi:qi + ln] != t)[0]
            last = 0
            for d in diff.tolist():
                run += d - last
                md.append(str(run)); md.append("ACGT"[int(t[d])])
                run, last = 0, d + 1
            run += ln - last
            nm += len(diff); qi += ln; ri += ln
        elif op == "I":
            qi += ln; nm += ln
        elif op == "D":
            md.append(str(run)); run = 0
            md.append("^" + "".join("ACGT"[int(c)] for c in ref_codes(pac, k0 + ri, ln)))
            ri += ln; nm += ln
        elif op == "S":
            qi += ln
        elif op != "H":
            raise ValueError("CIGAR operation %s" % op)
    md.append(str(run))
    return "".join(md), nm


def parse_cigar(s):
    return [(int(a), b) for a, b in CIG_RE.findall(s)]


def strip_tags(text):
    """SAM text without MD:Z and SA:Z fields."""
    return re.sub(r"\t(MD|SA):Z:[^\t\n]*", "", text)


def check_sam(text, pac, contig_off):
    """Every MD and SA of a SAM text against the recomputation; returns a list of problems (empty: all good)."""
    bad = []
    recs = [l.split("\t") for l in text.split("\n") if l and not l.startswith("@")]
    groups = []
    for f in recs:
        if not groups or groups[-1][0][0] != f[0]:
            groups.append([])
        groups[-1].append(f)
    for g in groups:
        mapped = [f for f in g if not int(f[1]) & 4]
        entries = []
        for f in mapped:
            tags = dict((t[:2], t[5:]) for t in f[11:])
            soft = f[5].replace("H", "S")
            entries.append("%s,%s,%s,%s,%s,%s;" % (f[2], f[3], "-" if int(f[1]) & 16 else "+", soft, f[4], tags.get("NM")))
        for i, f in enumerate(g):
            tags = dict((t[:2], t[5:]) for t in f[11:])
            if int(f[1]) & 4:
                if "MD" in tags or "SA" in tags:
                    bad.append((f[0], "tag on an unmapped record"))
                continue
            if "MD" in tags:
                md, nm = md_nm(pac, contig_off[f[2]] + int(f[3]) - 1, parse_cigar(f[5]), f[9])
                if not MD_RE.match(tags["MD"]):
                    bad.append((f[0], "MD not in SAM form: " + tags["MD"][:40]))
                if tags["MD"] != md:
                    bad.append((f[0], "MD %s... != %s..." % (tags["MD"][:40], md[:40])))
                if int(tags["NM"]) != nm:
                    bad.append((f[0], "NM %s != %d" % (tags["NM"], nm)))
            k = mapped.index(f)
            want = "".join(e for j, e in enumerate(entries) if j != k)
            if len(mapped) > 1 and tags.get("SA") != want:
                bad.append((f[0], "SA %s != %s" % (tags.get("SA"), want)))
            if len(mapped) < 2 and "SA" in tags:
                bad.append((f[0], "SA on a read with one record"))
    return bad


# ---- the result stream (include/lamsa_hp.h: lamsa_hp_result)
def split_events(s):
    """A read's stream with mismatch lists -> (the stream without them, [per record: list of event words])."""
    ev = []

    def strip(r):
        ev.append(r.mm)
        return r.hdr + r.cig
    return rebuild(s, strip, lists=True), ev


def stream_events(s, read, pac, seq_off):
    """The mismatch lists recomputed from a stream without them: per record (offset, chr, strand, CIGAR) against the read's
    codes (`read`, forward strand) and the .pac (`seq_off`: .pac offset of each contig)."""
    read = np.asarray(read, np.uint8)
    rc = revcomp_codes(read)
    ev = []
    for r in records(s):
        q = read if r.nstrand == 1 else rc
        w = np.asarray(r.cig, np.int64)
        op, ln = w & 0xf, w >> 4
        qs = np.concatenate([[0], np.cumsum(np.where((op == 0) | (op == 1) | (op == 4), ln, 0))])[:-1]
        rs = np.concatenate([[0], np.cumsum(np.where((op == 0) | (op == 2), ln, 0))])[:-1]
        m = op == 0
        n = int(ln[m].sum())
        start = np.repeat(np.cumsum(ln[m]) - ln[m], ln[m])                # index of each aligned base within the M runs
        j = np.arange(n) - start
        qi, ri = np.repeat(qs[m], ln[m]) + j, np.repeat(rs[m], ln[m]) + j
        t = ref_codes(pac, r.k0(seq_off), int(rs[-1] + (ln[-1] if op[-1] in (0, 2) else 0)) if len(op) else 0)
        d = np.nonzero(q[qi] != t[ri])[0]
        ev.append((ri[d] << 2 | t[ri[d]].astype(np.int64)).tolist())
    return ev
