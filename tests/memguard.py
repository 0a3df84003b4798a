"""Guarded arenas for the memory-contract tests (tests/test_gpu_memory_contract.py); holds no tests.

One allocation per call.  Every array of the call -- INPUTS INCLUDED -- is a sub-range of it with at least GUARD bytes of guard
in front and behind, at an address the caller chooses modulo 256.  Guards and the preset of the output regions come from
position-dependent patterns (a stray store of a plausible constant such as 0 or 0xEE cannot hide).  After the call `check`
compares every guard byte and every input byte with what was written and reports the first and last differing byte relative
to the nearest array: "32 bytes changed, 0 .. 31 bytes behind `d_ok`".

    a = DeviceArena([("d_scalars", sc_bytes, 16)], [("d_out", n * 64, 48)], fill=1)
    lib.bjj_mul_fixed_base_dev(h, a.ptr("d_scalars"), n, a.ptr("d_out"), None); ctx.sync()
    out = a.check()["d_out"]            # raises AssertionError on a changed guard or input byte

GUARD is 64 KiB: a kernel that steps one whole workgroup past the end of a batch (512 lanes x 128 bytes) still lands in memory
the test owns."""
import numpy as np

GUARD = 1 << 16
ALIGN = 256


def pattern(seed, lo, hi):
    """bytes lo .. hi - 1 of an endless position-dependent byte stream (one 64-bit mix per 8 bytes)"""
    if hi <= lo:
        return np.empty(0, np.uint8)
    w0, w1 = lo // 8, (hi + 7) // 8
    with np.errstate(over="ignore"):
        z = (np.arange(w0, w1, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFF)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
    return z.astype("<u8").view(np.uint8)[lo - 8 * w0:hi - 8 * w0]


GUARD_SEED = 0x6D656D67
FILL_SEEDS = {0: 0x0F111A, 1: 0x51DE0F}        # the two presets of the output regions ("fill")


class _Slot:
    def __init__(self, name, nbytes, off, data):
        self.name, self.nbytes, self.off, self.data, self.start = name, int(nbytes), int(off), data, None

    @property
    def end(self):
        return self.start + self.nbytes


class _Arena:
    """layout + image + check; the subclasses own the memory"""
    max_off_step = 16

    def __init__(self, inputs, outputs, fill=0):
        """inputs: [(name, bytes-like / uint8 array, off)], outputs: [(name, nbytes, off)]; off < 256 (device: a multiple of 16)"""
        self.slots = []
        for name, data, off in inputs:
            d = np.ascontiguousarray(data, np.uint8).reshape(-1)
            self.slots.append(_Slot(name, d.size, off, d))
        for name, nbytes, off in outputs:
            self.slots.append(_Slot(name, nbytes, off, None))
        for s in self.slots:
            assert 0 <= s.off < ALIGN and s.off % self.max_off_step == 0, (s.name, s.off)
        self.fill = fill
        self.total = sum(s.nbytes for s in self.slots) + (len(self.slots) + 1) * GUARD + (len(self.slots) + 1) * ALIGN
        self.base = self._allocate(self.total)
        cur = 0
        for s in self.slots:                                   # the smallest start >= cur + GUARD whose address is `off` mod 256
            p = cur + GUARD
            p += (s.off - (self.base + p)) % ALIGN
            s.start = p
            cur = s.end
        assert cur + GUARD <= self.total
        img = pattern(GUARD_SEED, 0, self.total).copy()
        for s in self.slots:
            img[s.start:s.end] = s.data if s.data is not None else pattern(FILL_SEEDS[fill], s.start, s.end)
        self.image = img
        self._upload(img)

    def ptr(self, name):
        s = self._slot(name)
        assert (self.base + s.start) % ALIGN == s.off
        return self.base + s.start

    def _slot(self, name):
        return next(s for s in self.slots if s.name == name)

    def check(self, outputs_unchanged=False):
        """every guard and input byte as written (outputs too with outputs_unchanged, the n = 0 rule); returns {output name: bytes}"""
        got = self._download()
        keep = np.ones(self.total, bool)
        if not outputs_unchanged:
            for s in self.slots:
                if s.data is None:
                    keep[s.start:s.end] = False
        bad = np.nonzero((got != self.image) & keep)[0]
        if bad.size:
            raise AssertionError(self._describe(bad))
        return {s.name: got[s.start:s.end].copy() for s in self.slots if s.data is None}

    def _describe(self, bad):
        msgs = []
        edges = [0] + [x for s in self.slots for x in (s.start, s.end)] + [self.total]
        for k in range(len(edges) - 1):                        # regions alternate: guard, array, guard, array, ..., guard
            lo, hi = edges[k], edges[k + 1]
            b = bad[(bad >= lo) & (bad < hi)]
            if not b.size:
                continue
            if k % 2:                                          # inside an array: an input (or an output of an n = 0 call)
                s = self.slots[k // 2]
                msgs.append("%d bytes changed inside %s `%s` (%d bytes at offset %d mod 256): first at byte %d, last at byte %d"
                            % (b.size, "input" if s.data is not None else "untouchable output", s.name, s.nbytes, s.off,
                               b[0] - lo, b[-1] - lo))
            else:
                before = self.slots[k // 2 - 1] if k else None
                after = self.slots[k // 2] if k // 2 < len(self.slots) else None
                parts = []
                if before is not None:
                    parts.append("%d .. %d bytes behind `%s`" % (b[0] - before.end, b[-1] - before.end, before.name))
                if after is not None:
                    parts.append("%d .. %d bytes in front of `%s`" % (after.start - b[-1], after.start - b[0], after.name))
                msgs.append("%d guard bytes changed, %s" % (b.size, " = ".join(parts)))
        return "; ".join(msgs)

    def close(self):
        pass


class DeviceArena(_Arena):
    """one torch uint8 allocation on cuda:0"""

    def _allocate(self, total):
        import torch
        self.buf = torch.empty(total, dtype=torch.uint8, device=torch.device("cuda", 0))
        return self.buf.data_ptr()

    def _upload(self, img):
        import torch
        self.buf.copy_(torch.from_numpy(img))
        torch.cuda.synchronize()

    def _download(self):
        import torch
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()


class HostArena(_Arena):
    """the same over a numpy array (pageable) or over Context.host_empty (pinned: pass the context).  The header sets no alignment
    rule for host pointers: any offset below 256 goes."""
    max_off_step = 1

    def __init__(self, inputs, outputs, fill=0, pinned_ctx=None):
        self.ctx = pinned_ctx
        super().__init__(inputs, outputs, fill)

    def _allocate(self, total):
        self.buf = self.ctx.host_empty(total) if self.ctx is not None else np.empty(total, np.uint8)
        return self.buf.ctypes.data

    def _upload(self, img):
        self.buf[:] = img

    def _download(self):
        return np.asarray(self.buf).copy()

    def close(self):
        if self.ctx is not None and self.buf is not None:
            self.ctx.host_free(self.buf)
        self.buf = None
