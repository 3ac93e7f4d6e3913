"""Operands with a huge leading dimension for tests/test_wide_stride_gpu.py: one canvas of R x LD floats (18 GiB), operands are
column windows of it.  A kernel then touches n x f elements whose byte offsets pass 2^31 (row 512), 2^32 (row 1024) and whose
element indices pass 2^31 (row 2048) and 2^32 (row 4096), without a big matrix.  A 2^32-byte wrap moves an access by exactly 1024
rows inside the same column window, i.e. to another row of the same operand: with different data in every row a wrong address reads
wrong values (or leaves a row unwritten / writes a row twice) instead of faulting.  Not a conftest: imported by the test module."""
import pytest
import torch

LD = 1 << 20                      # floats per canvas row: 4 MiB
R = 4608                          # 9 x 512 rows: 18 GiB
NEED_FREE = 24 << 30              # the canvas, the scan's temporaries and the compact operands
CHUNK_ROWS = 256                  # rows of the canvas scanned at a time (1 GiB; the comparison's temporary is 256 MiB)

# first row of the operand whose offset differs from the true one under each kind of truncation
BANDS = [(4096, ">= 4096 (unsigned 32-bit element index)"), (2048, ">= 2048 (signed 32-bit element index)"),
         (1024, ">= 1024 (unsigned 32-bit byte offset)"), (512, ">= 512 (signed 32-bit byte offset)"), (0, "< 512 (no wrap)")]


def band_of(row):
    return next(name for first, name in BANDS if row >= first)


class Canvas:
    """One contiguous allocation, never resized.  `reset()` fills it with NaN and forgets the windows handed out; every test input is
    finite, so after a call a non-NaN element outside the windows is a store that landed on a wrong address."""

    def __init__(self, dev):
        free, total = torch.cuda.mem_get_info(dev)
        if free < NEED_FREE:
            pytest.skip("%.1f GiB of device memory free, the wide-stride canvas needs %d GiB" % (free / 2 ** 30, NEED_FREE >> 30))
        self.dev = dev
        self.flat = torch.empty(R * LD, dtype=torch.float32, device=dev)
        self.windows = []
        self.inputs = []

    def reset(self):
        self.flat.fill_(float("nan"))
        self.windows = []
        self.inputs = []

    def window(self, rows, col0, f, ld=LD):
        """rows x f view with strides (ld, 1) starting at element col0.  ld = LD, col0 % 4 == 0: 16-byte aligned rows (the float4
        paths); ld = LD + 1 (the same storage, one row fewer) or col0 % 4 != 0: the scalar paths."""
        assert rows >= 0 and f > 0 and col0 >= 0 and col0 + f <= ld and (max(rows, 1) - 1) * ld + col0 + f <= self.flat.numel()
        w = self.flat.as_strided((rows, f), (ld, 1), col0)
        self.windows.append(w)
        return w

    def put(self, t, col0, ld=LD, const=True):
        """A window holding a copy of the 2-d tensor t (strided copy_).  const: an input that no call may change -- stray_writes()
        compares it with t again (t itself must stay unchanged); False for operands updated in place."""
        w = self.window(t.shape[0], col0, t.shape[1], ld)
        w.copy_(t)
        if const:
            self.inputs.append((w, t))
        return w

    def stray_writes(self):
        """Non-NaN elements of the canvas outside the windows handed out since reset() (which must not overlap), plus the elements
        of input windows that no longer equal their (finite) source: a store that landed inside an input."""
        total = 0
        step = CHUNK_ROWS * LD
        for a in range(0, self.flat.numel(), step):
            c = self.flat[a:a + step]
            total += int((c == c).sum())
        inside = sum(int((w == w).sum()) for w in self.windows)
        changed = sum(int((w != t).sum()) for w, t in self.inputs)
        return total - inside + changed


def by_band(got, want):
    """None when got and want hold the same bits, else a message naming the first mismatching row and its band."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if torch.equal(g, w):
        return None
    bad = (g != w).reshape(g.shape[0], -1).any(1)
    rows = torch.nonzero(bad).flatten()
    first = int(rows[0])
    per = {}
    for r in rows.tolist():
        per[band_of(r)] = per.get(band_of(r), 0) + 1
    return "first mismatching row %d: band %s; %d rows differ %s" % (first, band_of(first), rows.numel(), per)


def assert_same_bits(got, want, what=""):
    msg = by_band(got, want)
    assert msg is None, "%s: strided result differs from the compact one -- %s" % (what, msg)
