"""An independent checker for the FM-index search (lamsa_hp_fm_search, include/lamsa_hp.h): from <ref>.pac and the contig table of
<ref>.ann alone it builds the doubled text (forward reference + reverse complement) and its suffix array with numpy (prefix doubling),
and answers row intervals and text positions in row order.  Row 0 is the sentinel suffix, row r >= 1 the r-th smallest suffix.
It shares no code with the product: no BWT, no occurrence counts, no sampled suffix array."""
import numpy as np


def read_ann(prefix):
    """(l_pac, [(name, offset, length)]) from <prefix>.ann (bns_restore, src/bntseq.c: two lines per contig)."""
    lines = open(prefix + ".ann").read().split("\n")
    l_pac, n_seqs = int(lines[0].split()[0]), int(lines[0].split()[1])
    contigs = []
    for i in range(n_seqs):
        name = lines[1 + 2 * i].split()[1]
        off, ln = lines[2 + 2 * i].split()[:2]
        contigs.append((name, int(off), int(ln)))
    assert sum(c[2] for c in contigs) == l_pac
    return l_pac, contigs


def doubled_text(prefix):
    l_pac, _ = read_ann(prefix)
    pac = np.fromfile(prefix + ".pac", np.uint8)
    k = np.arange(l_pac, dtype=np.int64)
    fwd = (pac[k >> 2] >> ((~k & 3) << 1).astype(np.uint8)) & 3
    return np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)


def suffix_array(text):
    """Suffix array by prefix doubling; a suffix that is a prefix of another one comes first."""
    n = len(text)
    rank = text.astype(np.int64)
    h = 1
    while True:
        nxt = np.zeros(n, np.int64)
        if h < n:
            nxt[:n - h] = rank[h:] + 1
        key = rank * (int(rank.max()) + 2) + nxt
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        new = np.zeros(n, np.int64)
        new[sa] = np.concatenate([[0], np.cumsum(ks[1:] != ks[:-1])])
        rank = new
        if int(rank.max()) == n - 1:
            return sa.astype(np.int64)
        h *= 2


class FmCheck:
    def __init__(self, prefix):
        self.text = doubled_text(prefix)
        self.n = len(self.text)
        self.sa = suffix_array(self.text)                  # sa[r - 1]: text position of row r
        self.primary = int(np.nonzero(self.sa == 0)[0][0]) + 1
        self._keys = {}

    def row_value(self, row):
        return int(self.sa[row - 1])

    def _text_keys(self, k):
        """Per row 1..n in row order: the first min(k, 32) and the next k - 32 symbols of its suffix as integers; rows whose suffix is
        shorter than k are left out.  Returns (rows, key1, key2)."""
        if k not in self._keys:
            t = np.concatenate([self.text, np.zeros(k, np.uint8)]).astype(np.uint64)
            k1, k2 = min(k, 32), max(k - 32, 0)
            a = np.zeros(self.n, np.uint64); b = np.zeros(self.n, np.uint64)
            for i in range(k1):
                a = (a << np.uint64(2)) | t[i:i + self.n]
            for i in range(k2):
                b = (b << np.uint64(2)) | t[32 + i:32 + i + self.n]
            ok = self.sa + k <= self.n
            rows = np.nonzero(ok)[0] + 1
            p = self.sa[ok]
            self._keys[k] = (rows, a[p], b[p])
        return self._keys[k]

    def intervals(self, kmers, k):
        """kmers: [n, k] uint8 codes 0..4 -> (lo, hi) uint64 arrays, inclusive rows; (1, 0) for a k-mer that does not occur or holds a 4."""
        kmers = np.asarray(kmers, np.uint8).reshape(-1, k)
        n = len(kmers)
        lo = np.ones(n, np.uint64); hi = np.zeros(n, np.uint64)
        rows, key1, key2 = self._text_keys(k)
        k1, k2 = min(k, 32), max(k - 32, 0)
        q = kmers.astype(np.uint64)
        a = np.zeros(n, np.uint64); b = np.zeros(n, np.uint64)
        for i in range(k1):
            a = (a << np.uint64(2)) | (q[:, i] & np.uint64(3))
        for i in range(k2):
            b = (b << np.uint64(2)) | (q[:, 32 + i] & np.uint64(3))
        valid = (kmers <= 3).all(axis=1)
        x = np.searchsorted(key1, a, "left"); y = np.searchsorted(key1, a, "right")
        for j in range(n):
            if not valid[j] or x[j] == y[j]:
                continue
            s, e = int(x[j]), int(y[j])
            if k2:
                sub = key2[s:e]
                s, e = s + int(np.searchsorted(sub, b[j], "left")), s + int(np.searchsorted(sub, b[j], "right"))
                if s == e:
                    continue
            assert int(rows[e - 1]) - int(rows[s]) == e - 1 - s          # the rows of one k-mer are neighbours
            lo[j] = rows[s]; hi[j] = rows[e - 1]
        return lo, hi

    def search(self, seq, win_off, k, max_occ):
        """What lamsa_hp_fm_search answers: (kmer_off, lo, hi, pos_off, pos)."""
        seq = np.asarray(seq, np.uint8); win_off = np.asarray(win_off, np.int64)
        kmer_off = [0]; parts = []
        for w in range(len(win_off) - 1):
            win = seq[win_off[w]:win_off[w + 1]]
            m = max(len(win) - k + 1, 0)
            kmer_off.append(kmer_off[-1] + m)
            if m:
                parts.append(np.lib.stride_tricks.sliding_window_view(win, k))
        kmers = np.concatenate(parts) if parts else np.zeros((0, k), np.uint8)
        lo, hi = self.intervals(kmers, k)
        cnt = (hi + np.uint64(1) - lo).astype(np.int64)
        cnt[hi < lo] = 0
        take = np.where((cnt >= 1) & (cnt <= max_occ), cnt, 0)
        pos_off = np.concatenate([[0], np.cumsum(take)]).astype(np.int64)
        pos = np.zeros(int(pos_off[-1]), np.uint64)
        for j in np.nonzero(take)[0]:
            pos[pos_off[j]:pos_off[j + 1]] = self.sa[int(lo[j]) - 1:int(hi[j])]
        return np.asarray(kmer_off, np.int64), lo, hi, pos_off, pos, cnt
