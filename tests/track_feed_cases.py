"""Cases and the numpy restatement of sda_gather_windows (training batches gathered from resident speech tracks), shared by
tests/test_track_feed_cpu.py and tests/test_track_feed_gpu.py.

The kernel moves bytes, so a table here is an array of unsigned integers of the element's width — (L, Cp) uint16 for bf16 / fp16
storage, uint32 for fp32 — with the channel padding [F, Cp) zero, as a WindowBank keeps it, and every valid element non-zero.
Valid elements are distinct: a seeded permutation of 1 ... n for 32-bit elements; for 16-bit elements, whose 65535 non-zero
patterns case (c) outruns, one independent permutation of 1 ... 65535 after the other (cases a and b fit into the first and are
distinct throughout; in case c rows of one permutation share no value and rows of different ones agree at a column once in
65535), so that a misplaced, shifted or dropped row cannot go unnoticed.

The restatement returns the WHOLE destination, rows_alloc(B, T) x Cp: pad rows, windows, slack.  It starts from FILL, a NaN bit
pattern standing for uninitialised memory, which a correct gather overwrites everywhere and a planted bug leaves showing.
"""
import numpy as np

PAD = 16                       # SDA_ROW_PAD
SLACK = PAD + 128 + 2 * PAD    # rows behind the last sample: sda_rows_alloc(B, T) - B * (T + PAD)
FILL = {np.dtype(np.uint16): 0x7FC1, np.dtype(np.uint32): 0x7FC00001}       # NaN patterns: 0x7FC1 is one in bf16 and in fp16

BUGS = ("pad rows unwritten", "slack unwritten", "start off by one", "idx as the table row", "last row of the last sample dropped",
        "sample stride T", "channel padding not carried")


def pad64(c: int) -> int:
    return (c + 63) // 64 * 64


def rows_alloc(B: int, T: int) -> int:
    return B * (T + PAD) + SLACK


def make_table(L: int, F: int, utype, seed: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    n = L * F
    if np.dtype(utype) == np.uint32:
        vals = rng.permutation(n).astype(np.uint32) + 1
    else:
        vals = np.concatenate([rng.permutation(65535) + 1 for _ in range((n + 65534) // 65535)])[:n].astype(np.uint16)
    table = np.zeros((L, pad64(F)), dtype=utype)
    table[:, :F] = vals.reshape(L, F)
    return table


def case(name: str, utype=np.uint16) -> dict:
    """F, T, track lengths, the candidates' global table rows `starts` (int32) and the batch `idx` (int64) of case a1, a7, b or c."""
    if name in ("a1", "a7"):
        # Cp = 64: one 128-byte row in 16-bit storage.  Both tracks' first and last legal starts; 27 + 5 = 32 ends the table.
        F, T, lens = 40, 5, (23, 9)
        starts = [0, 18, 7, 23, 27, 11]
        idx = [4] if name == "a1" else [4, 1, 1, 0, 5, 3, 2]                # duplicates, shuffled order
    elif name == "b":
        # Cp = 128, a window every 3 rows: neighbouring candidates share 37 of their 40 rows
        F, T, lens = 70, 40, (61, 97, 52)
        starts, row0 = [], 0
        for n in lens:
            starts += [row0 + s for s in sorted(set(range(0, n - T + 1, 3)) | {n - T})]      # hop 3, and the last legal start
            row0 += n
        idx = list(np.random.RandomState(5).randint(0, len(starts), size=9))
        idx[3] = idx[0]                                                     # a duplicate for certain
        idx[8] = len(starts) - 1                                            # the table's final rows
    elif name == "c":
        # the workload's sample: 360 rows of 2 KiB (16-bit).  46080 vectors over 23 workgroups: the unrolled loop runs once and
        # its tail three or four times per lane, and more than one workgroup works on a sample
        F, T, lens = 1024, 360, (400, 380)
        starts = [0, 40, 420, 400]                                          # 420 + 360 = 780 ends the table
        idx = [2, 0, 1]
    else:
        raise KeyError(name)
    L = int(sum(lens))
    starts = np.asarray(starts, dtype=np.int32)
    assert starts.min() >= 0 and starts.max() + T <= L and (starts + T == L).any() and (starts == 0).any()
    return {"name": name, "F": F, "T": T, "lens": lens, "Cp": pad64(F), "table": make_table(L, F, utype, seed=11 + len(name) + F),
            "starts": starts, "idx": np.asarray(idx, dtype=np.int64), "B": len(idx)}


CASES = ("a1", "a7", "b", "c")


def gather_windows_ref(table: np.ndarray, starts: np.ndarray, idx: np.ndarray, T: int) -> np.ndarray:
    """What one sda_gather_windows launch leaves in dst, every row of it."""
    L, Cp = table.shape
    B = len(idx)
    out = np.full((rows_alloc(B, T), Cp), FILL[table.dtype], dtype=table.dtype)
    for b, m in enumerate(idx):
        r0 = b * (T + PAD)
        out[r0: r0 + PAD] = 0
        s = int(starts[m]) if 0 <= m < len(starts) else -1
        if 0 <= s <= L - T:
            out[r0 + PAD: r0 + PAD + T] = table[s: s + T]
        else:
            out[r0 + PAD: r0 + PAD + T] = 0
    out[B * (T + PAD):] = 0
    return out


def gather_windows_bugged(table: np.ndarray, starts: np.ndarray, idx: np.ndarray, T: int, F: int, bug: str) -> np.ndarray:
    """A copy of the restatement with ONE of BUGS planted (valid candidates only)."""
    assert bug in BUGS
    L, Cp = table.shape
    B = len(idx)
    stride = T if bug == "sample stride T" else T + PAD
    out = np.full((rows_alloc(B, T), Cp), FILL[table.dtype], dtype=table.dtype)
    for b, m in enumerate(idx):
        r0 = b * stride
        if bug != "pad rows unwritten":
            out[r0: r0 + PAD] = 0
        s = int(m) if bug == "idx as the table row" else int(starts[m])
        if bug == "start off by one":
            s += 1
        n = T - 1 if (bug == "last row of the last sample dropped" and b == B - 1) else T
        rows = table[s: s + n]                                              # (a start off by one may run off the table: fewer rows)
        cols = F if bug == "channel padding not carried" else Cp
        out[r0 + PAD: r0 + PAD + len(rows), :cols] = rows[:, :cols]
    if bug != "slack unwritten":
        out[B * (T + PAD):] = 0
    return out
