"""An independent checker for seeding in the FM index (lamsa_hp_fm_seed, include/lamsa_hp.h).  Rows and text positions come from
tests/fmcheck.py (a suffix array of the doubled text made with numpy, every seed searched as a window of its own); the rules that turn a
located row into a hit record -- strand, contig, bounds, the over-max slot -- are restated here in numpy from the header's definition.
It shares no code with the product.  It yields the expected lamsa_hp_batch arrays, counts the classes of seeds and rows the tests want
to have seen, and can write the batch as a GEM map text in the fixtures' format for a run with -N."""
import numpy as np

import fmcheck

NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    NT4[ord(_c)] = _i; NT4[ord(_c.lower())] = _i


def read_fasta(path):
    """[(name, codes)] of a FASTA file, gzipped or not (the name up to the first blank)."""
    import gzip
    out, name, parts = [], None, []
    for line in (gzip.open(path, "rt") if path.endswith(".gz") else open(path)):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if name is not None:
                out.append((name, NT4[np.frombuffer("".join(parts).encode(), np.uint8)]))
            name, parts = line[1:].split()[0] if len(line) > 1 else "", []
        elif name is not None:
            parts.append(line)
    if name is not None:
        out.append((name, NT4[np.frombuffer("".join(parts).encode(), np.uint8)]))
    return out


class Expected:
    """The arrays of a lamsa_hp_batch (word form: cig / h_cig_off, and cig8 for the compact form), the reference arrays reflib's oracle
    wants when given (pac, l_pac, seq_off, seq_len), and per seed what the map writer and the class counters need."""


def expected(chk, contigs, reads, seed_len, seed_step, max_hits, prefix=None):
    """chk: fmcheck.FmCheck of the index; contigs: [(name, offset, length)] (fmcheck.read_ann); reads: list of uint8 code arrays."""
    l_pac = chk.n // 2
    offs = np.array([c[1] for c in contigs], np.int64); lens = np.array([c[2] for c in contigs], np.int64)
    n = len(reads)
    L = np.array([len(r) for r in reads], np.int64)
    seed_all = np.where(L < seed_len, 0, 1 + (L - seed_len) // seed_step).astype(np.int64)
    last_len = L - seed_len - (seed_all - 1) * seed_step
    wins = [np.asarray(reads[r], np.uint8)[i * seed_step:i * seed_step + seed_len] for r in range(n) for i in range(int(seed_all[r]))]
    N = len(wins)
    owner = np.repeat(np.arange(n), seed_all); first = np.concatenate([[0], np.cumsum(seed_all)])
    sid = np.arange(N) - first[owner] + 1                                   # 1-based seed index
    seq = np.concatenate(wins + [np.zeros(16, np.uint8)]).astype(np.uint8)
    win_off = np.arange(N + 1, dtype=np.int64) * seed_len
    _, lo, hi, pos_off, pos, cnt = chk.search(seq, win_off, seed_len, 1 << 40) if N else (None, np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.int64))
    over = cnt > max_hits
    # every row of every seed, in seed order and row order
    row_seed = np.repeat(np.arange(N), cnt)
    p = pos.astype(np.int64)
    is_rev = p >= l_pac
    f = np.where(is_rev, 2 * l_pac - 1 - p, p)
    c = np.searchsorted(offs, f, "right") - 1
    hpos = f - offs[c] + 1 - np.where(is_rev, seed_len - 1, 0)
    inside = (hpos >= 1) & (hpos + seed_len - 1 <= lens[c])
    keep = inside & ~over[row_seed]
    kept = np.bincount(row_seed[keep], minlength=N).astype(np.int64) if N else np.zeros(0, np.int64)
    slot = (kept > 0) | over
    E = Expected()
    E.n_reads = n
    E.read_off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    E.read_seq = np.concatenate([np.asarray(r, np.uint8) for r in reads] + [np.zeros(16, np.uint8)]).astype(np.uint8)
    E.seed_all = seed_all.astype(np.int32); E.last_len = last_len.astype(np.int32)
    E.seed_off = np.concatenate([[0], np.cumsum(slot)])[first].astype(np.int64)
    E.seed_id = sid[slot].astype(np.int32)
    E.hit_off = np.concatenate([[0], np.cumsum(kept[slot])]).astype(np.int64)
    E.h_pos = hpos[keep].astype(np.int64); E.h_chr = (c[keep] + 1).astype(np.int32); E.h_strand = np.where(is_rev[keep], -1, 1).astype(np.int8)
    nh = len(E.h_pos)
    E.h_nm = np.zeros(nh, np.int16); E.h_len_dif = np.zeros(nh, np.int16); E.h_cig_n = np.ones(nh, np.uint8)
    E.h_cig_off = np.arange(nh, dtype=np.int32); E.cig = np.full(nh, seed_len << 4, np.int32); E.cig8 = np.full(nh, seed_len, np.uint8)
    E.n_slots = int(slot.sum()); E.n_hits = nh; E.n_rows_located = int(cnt[~over].sum())
    if prefix is not None:
        E.pac = np.fromfile(prefix + ".pac", np.uint8); E.l_pac = l_pac; E.seq_off = offs.copy(); E.seq_len = lens.astype(np.int32)
    # for the map writer: every row of a seed with a slot (an over-max seed lists all its rows, so that the parser empties it)
    E._map = dict(first=first, sid=sid, wins=wins, cnt=cnt, over=over, slot=slot, row_off=np.concatenate([[0], np.cumsum(cnt)]), keep=keep, c=c, is_rev=is_rev, hpos=hpos)
    # the classes of seeds and rows (tests/test_seed_*.py assert that the hand-placed reads meet every one)
    has4 = np.array([bool((w > 3).any()) for w in wins], bool) if N else np.zeros(0, bool)
    located = ~over[row_seed]
    plus_kept = np.bincount(row_seed[keep & ~is_rev], minlength=N) if N else np.zeros(0, np.int64)
    minus_kept = np.bincount(row_seed[keep & is_rev], minlength=N) if N else np.zeros(0, np.int64)
    last_c = len(contigs) - 1
    E.classes = dict(
        a_unique_plus=int(((cnt == 1) & (plus_kept == 1)).sum()), b_unique_minus=int(((cnt == 1) & (minus_kept == 1)).sum()),
        c_absent=int(((cnt == 0) & ~has4).sum()), d_has_n=int(has4.sum()), e_at_max=int((cnt == max_hits).sum()), f_over_max=int(over.sum()),
        g_contig_boundary=int((located & ~inside & ~is_rev & (c < last_c)).sum()), h_text_middle=int((located & (p < l_pac) & (p + seed_len > l_pac)).sum()),
        i_minus_into_previous=int((located & is_rev & (hpos < 1)).sum()), j_first_base=int((keep & (hpos == 1)).sum()),
        j_last_base=int((keep & (hpos + seed_len - 1 == lens[c])).sum()), k_both_strands=int(((plus_kept > 0) & (minus_kept > 0)).sum()),
        l_all_dropped=int(((cnt >= 1) & ~over & (kept == 0)).sum()))
    return E


ARRAYS = ("read_off", "seed_all", "last_len", "seed_off", "seed_id", "hit_off", "h_pos", "h_chr", "h_strand", "h_nm", "h_len_dif", "h_cig_n", "cig8")


def assert_batch(got, want, what):
    """got: dict of numpy arrays as LamsaHp.fm_seed / seedlib.fm_seed_lib return them; word for word the checker's."""
    assert got["n_reads"] == want.n_reads and got["n_cig"] == want.n_hits, (what, got["n_cig"], want.n_hits)
    for name in ARRAYS:
        g, w = np.asarray(got[name]), np.asarray(getattr(want, name))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:5])
    assert got["h_cig_off"] is None and got["cig"] is None, what


def as_batch(got, want):
    """The arrays a call returned as an object reflib.emu_streams / LamsaHp.align_batch take (compact form), with the reference arrays of `want`."""
    B = Expected()
    B.n_reads = got["n_reads"]
    B.read_seq = want.read_seq
    for name in ARRAYS:
        a = got[name]
        setattr(B, name, a if len(a) else np.zeros(4, a.dtype)[:0])
    B.h_cig_off = None; B.cig = None
    for name in ("pac", "l_pac", "seq_off", "seq_len"):
        if hasattr(want, name):
            setattr(B, name, getattr(want, name))
    return B


def write_map(path, names, want, contigs, seed_len, seed_step):
    """The expected batch as a GEM map text in the fixtures' format, one line per seed: name_i:offset, the seed, an empty field, the
    number of hits, then chr:strand:pos:LEN,... in row order; '-' for a seed without a slot; all rows of an over-max seed."""
    m = want._map
    acgtn = "ACGTN"
    with open(path, "w") as fp:
        for j in range(len(m["sid"])):
            r = int(np.searchsorted(m["first"], j, "right") - 1)
            i = int(m["sid"][j]) - 1
            a, b = int(m["row_off"][j]), int(m["row_off"][j + 1])
            rows = [t for t in range(a, b) if m["over"][j] or m["keep"][t]] if m["slot"][j] else []
            hits = ",".join("%s:%s:%d:%d" % (contigs[int(m["c"][t])][0], "-" if m["is_rev"][t] else "+", int(m["hpos"][t]), seed_len) for t in rows)
            fp.write("%s_%d:%d\t%s\t\t%d\t%s\n" % (names[r], i, i * seed_step, "".join(acgtn[x] for x in m["wins"][j]), len(rows), hits if rows else "-"))
