"""TEST INFRASTRUCTURE ONLY -- the plain-python model of the paged pool (oracle.kv_paged.PagedPoolModel, imported as it
is) with per-block share counts: ``share[b]`` = holders of block ``b`` minus one, ``fork`` and the reference-counted
``release``, with the sequential semantics ll_kv_paged_fork / ll_kv_paged_release_shared are held to (csrc/kv_paged.hip).
``fork`` records the ``(source block, new block, rows)`` copies it asks for; ``check_invariants`` is what must hold
after every operation, for the model and for the device state alike."""

from __future__ import annotations

import numpy as np

from oracle.kv_paged import PagedPoolModel


class SharedPagedPoolModel(PagedPoolModel):
    def __init__(self, num_blocks, block_size, max_requests, max_seq_len):
        super().__init__(num_blocks, block_size, max_requests, max_seq_len)
        self.share = np.zeros(num_blocks, dtype=np.int32)
        self.copies = []          # (source block, new block, rows) of the last accepted fork

    def fork(self, src, dst, lens):
        """Call order i = 0 .. n-1.  Refused as a whole (bit 4) if any dst holds a block, is listed twice or is a source of
        the same call, or any length is < 1 or reaches beyond the source's blocks; refused as a whole (bit 1) if the partial
        blocks outnumber the free blocks."""
        bs = self.bs
        self.copies = []
        if len(set(dst)) != len(dst) or set(dst) & set(src):
            self.err |= 4
            return False
        for s, d, ln in zip(src, dst, lens):
            if self.req_blocks[d] != 0 or ln < 1 or (ln + bs - 1) // bs > self.req_blocks[s]:
                self.err |= 4
                return False
        need = [1 if ln % bs else 0 for ln in lens]
        if sum(need) > self.free:
            self.err |= 1
            return False
        for s, d, ln, nd in zip(src, dst, lens, need):
            full, rem = ln // bs, ln % bs
            for j in range(full):
                b = int(self.block_table[s, j])
                self.block_table[d, j] = b
                self.share[b] += 1
            if rem:
                self.free -= 1
                nb = self.stack[self.free]
                self.block_table[d, full] = nb
                self.copies.append((int(self.block_table[s, full]), nb, rem))
            self.req_blocks[d] = full + nd
            for p in range(ln):
                self.token_table[d, p] = int(self.block_table[d, p // bs]) * bs + p % bs
        return True

    def release(self, req_idx):
        for r in req_idx:
            for j in range(int(self.req_blocks[r])):
                b = int(self.block_table[r, j])
                if self.share[b] > 0:
                    self.share[b] -= 1        # someone else still holds it
                else:
                    self.stack[self.free] = b  # last holder
                    self.free += 1
            self.req_blocks[r] = 0


def check_invariants(nb, free, stack, req_blocks, block_table, share):
    """free blocks + distinct held blocks = nb - 1; share[b] = holders - 1 (0 if free); the free stack holds no held block
    and no block twice; nothing names the junk block."""
    holders = np.zeros(nb, dtype=np.int64)
    for r in range(len(req_blocks)):
        row = [int(b) for b in block_table[r, : int(req_blocks[r])]]
        assert len(set(row)) == len(row), ("a request holds a block twice", r, row)
        for b in row:
            assert 0 <= b < nb - 1, ("a request holds the junk block or a block outside the pool", r, b)
            holders[b] += 1
    held = set(int(b) for b in np.nonzero(holders)[0])
    on_stack = [int(b) for b in stack[:free]]
    assert len(set(on_stack)) == len(on_stack), "a block is on the free stack twice"
    assert not held & set(on_stack), ("a held block is on the free stack", held & set(on_stack))
    assert free + len(held) == nb - 1, (free, len(held), nb)
    want = np.where(holders > 0, holders - 1, 0)
    assert np.array_equal(np.asarray(share, dtype=np.int64), want), (share, want)


def check_model(m: SharedPagedPoolModel):
    check_invariants(m.nb, m.free, m.stack, m.req_blocks, m.block_table, m.share)


class RandomOps:
    """The random admit / fork / append / release sequence the CPU and the GPU tests drive: yields ``(op, args)`` and keeps
    the host's view of every request's length.  Forks: several children per call, the same source repeated, chains (a
    child is a later source), lengths below the source's length, on and off block boundaries.  Releases: parents before
    children, children before parents, all holders of a block in one call."""

    def __init__(self, seed, bs, max_req, max_len):
        self.rng = np.random.default_rng(seed)
        self.bs, self.max_req, self.max_len = bs, max_req, max_len
        self.lens = np.zeros(max_req, dtype=np.int64)
        self.live = set()

    def next(self):
        rng, bs = self.rng, self.bs
        idle = [r for r in range(self.max_req) if r not in self.live]
        live = sorted(self.live)
        op = int(rng.integers(0, 12))
        if op < 2 and idle:
            k = int(rng.integers(1, min(3, len(idle)) + 1))
            reqs = [int(r) for r in rng.choice(idle, k, replace=False)]
            ln = [int(rng.integers(1, max(2, self.max_len // 2))) for _ in reqs]
            return "admit", (reqs, ln, max(ln) + int(rng.integers(0, 3)))
        if op < 5 and idle and live:
            k = int(rng.integers(1, min(5, len(idle)) + 1))
            dst = [int(r) for r in rng.choice(idle, k, replace=False)]
            src = [int(live[int(rng.integers(0, len(live)))]) for _ in dst] if rng.integers(0, 2) else \
                [int(live[int(rng.integers(0, len(live)))])] * k
            ln = []
            for s in src:
                full = int(self.lens[s])
                kind = int(rng.integers(0, 3))
                v = full if kind == 0 else int(rng.integers(1, full + 1))
                if kind == 2 and full >= bs:
                    v = (v // bs) * bs or bs              # on a block boundary
                ln.append(v)
            return "fork", (src, dst, ln)
        if op < 9 and live:
            reqs = [r for r in live if rng.integers(0, 2) and self.lens[r] + 1 <= self.max_len]
            if reqs:
                return "append", (reqs, [int(self.lens[r] + 1) for r in reqs])
        if live:
            k = int(rng.integers(1, min(4, len(live)) + 1))
            return "release", ([int(r) for r in rng.choice(live, k, replace=False)],)
        return "noop", ()

    # what the caller reports back once the pool (model) has answered
    def admitted(self, reqs, ln, req_blocks):
        for r, n in zip(reqs, ln):
            if int(req_blocks[r]) * self.bs >= n:
                self.live.add(r)
                self.lens[r] = n

    def forked(self, dst, ln):
        for d, n in zip(dst, ln):
            self.live.add(d)
            self.lens[d] = n

    def appended(self, reqs, new, req_blocks):
        for r, n in zip(reqs, new):
            if int(req_blocks[r]) * self.bs >= n:
                self.lens[r] = n

    def released(self, reqs):
        for r in reqs:
            self.live.discard(r)
            self.lens[r] = 0
