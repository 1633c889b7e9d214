"""Pointer tables over padded buffers with guard words, for the raw C ABI tests -- test helper (the table
builder of the test_abi_unaligned_multi_segment tests as one class, with an element offset per (array,
segment, row) instead of one per array).

Every array `k` is one [n, stride] device buffer filled with its guard word.  Row r holds its copy of
segment s at element  base[s] + off(k, s, r), base[s] a multiple of 8 elements (16-byte aligned for 2- and
4-byte elements alike) and 0 <= off < 8, so off alone decides the alignment of the (segment, row) pointer;
at least 8 guard elements lie before and after every segment, a zero-length one included."""
import numpy as np
import torch

GUARD = {np.dtype(np.float32): np.float32(777.25), np.dtype(np.uint16): np.uint16(0x4D4D)}


class PaddedTables:
    def __init__(self, n, lens, dtypes, off):
        """dtypes: array name -> np.float32 / np.uint16; off(k, s, r) -> element offset in [0, 8)"""
        self.n, self.lens, self.P = n, [int(v) for v in lens], int(sum(lens))
        self.dtypes = {k: np.dtype(d) for k, d in dtypes.items()}
        self.base, at = [], 8
        for length in self.lens:
            self.base.append(at)
            at += (length + 7) // 8 * 8 + 16                     # the offset (< 8) and 8 guard elements at least
        self.stride = at
        self.start = {k: np.array([[self.base[s] + int(off(k, s, r)) for s in range(len(self.lens))]
                                   for r in range(n)], np.int64) for k in self.dtypes}
        for k in self.dtypes:
            assert ((self.start[k] - np.array(self.base)) >= 0).all() and ((self.start[k] - np.array(self.base)) < 8).all()
        self.inside = {}
        self.dev = {}
        for k, dt in self.dtypes.items():
            m = np.zeros((n, self.stride), bool)
            for r in range(n):
                for s, length in enumerate(self.lens):
                    m[r, self.start[k][r, s]:self.start[k][r, s] + length] = True
            assert int(m.sum()) == n * self.P
            self.inside[k] = m
            host = np.full((n, self.stride), GUARD[dt], dt)
            self.dev[k] = torch.from_numpy(host.view(np.int16) if dt == np.uint16 else host).cuda()
            assert self.dev[k].data_ptr() % 16 == 0 and (self.stride * dt.itemsize) % 16 == 0

    def ptrs(self, k):
        """rows x segments device addresses (the layouts' `*_ptrs` lists)"""
        size = self.dtypes[k].itemsize
        return [[self.dev[k][r].data_ptr() + size * int(self.start[k][r, s]) for s in range(len(self.lens))]
                for r in range(self.n)]

    def host(self, k):
        torch.cuda.synchronize()
        a = self.dev[k].cpu().numpy()
        return a.view(np.uint16) if self.dtypes[k] == np.uint16 else a

    def put(self, k, values):
        """values [n, sum(lens)]: the segments side by side; guard words rewritten too"""
        dt = self.dtypes[k]
        a = np.full((self.n, self.stride), GUARD[dt], dt)
        a[self.inside[k]] = np.ascontiguousarray(values, dt).reshape(-1)       # row-major: segments in order
        self.dev[k].copy_(torch.from_numpy(a.view(np.int16) if dt == np.uint16 else a))

    def get(self, k):
        """[n, sum(lens)]: the segments side by side"""
        return self.host(k)[self.inside[k]].reshape(self.n, self.P)

    def guards_intact(self, k):
        a = self.host(k)
        g = GUARD[self.dtypes[k]]
        return bool((a[~self.inside[k]].view(np.uint32 if a.dtype == np.float32 else np.uint16) ==
                     np.array([g]).view(np.uint32 if a.dtype == np.float32 else np.uint16)[0]).all())
