"""Byte model and seeded op generator for queued-I/O tests (hs.IoQueue).

The model is a ``bytearray`` the size of the bdev: the plain reference
every engine is compared with, byte for byte.

Semantics encoded here:
  * ops inside one ``run()`` have NO mutual ordering (the batched engine
    executes a whole run as one launch, resident engines serve tiles on
    many waves, and ``flush`` is a completion marker, not a barrier), so
    a write or fill must share no byte with any other op of its run
    (two reads may overlap) — ``apply`` refuses anything else, and the
    generator only produces pairwise-disjoint runs;
  * ordering holds across ``run()`` calls: a run sees everything that
    earlier runs completed;
  * a request is valid iff it is a flush, or its length is a non-zero
    multiple of the block size at a block-aligned offset inside the
    bdev; invalid requests complete with -22 and change nothing.

Op tuples are the ones ``IoQueue.run`` takes:
  ("read", offset, length) / ("write", offset, data) /
  ("fill", offset, length, value) / ("flush",)
"""

import random

TILE = 4096  # every engine splits a request into 4 KiB descriptors

STATUS_OK = 0
STATUS_INVALID = -22

# Lengths where a tile loop can go wrong: a sub-tile request, two lanes'
# worth more or less than a tile, one block short of a tile, exactly one
# tile, a tile plus one block, two tiles plus a block, and a multi-tile
# request with a ragged three-block tail.
EDGE_LENGTHS = (512, 1024, 1536, 3584, 4096, 4608, 8192 + 512, 65536 + 1536)


def op_length(op):
    if op[0] == "write":
        return len(op[2])
    if op[0] == "flush":
        return 0
    return op[2]


def op_range(op):
    """[start, end) of the bdev bytes an op names; None for a flush."""
    if op[0] == "flush":
        return None
    return op[1], op[1] + op_length(op)


def op_tiles(op):
    """Descriptors (4 KiB tiles) the engines expand this op into."""
    return -(-op_length(op) // TILE)


def assert_disjoint(ops):
    """Raise ValueError if a write or fill of one run shares a byte with
    any other op of that run (two reads may overlap: order between
    them cannot matter)."""
    spans = sorted((r[0], r[1], i) for i, r in
                   ((i, op_range(op)) for i, op in enumerate(ops))
                   if r is not None and r[1] > r[0])
    any_end, any_idx = 0, None        # furthest end of any op so far
    store_end, store_idx = 0, None    # furthest end of a write/fill
    for start, end, i in spans:
        stores = ops[i][0] != "read"
        clash = None
        if stores and start < any_end:
            clash = any_idx
        elif not stores and start < store_end:
            clash = store_idx
        if clash is not None:
            raise ValueError(
                f"ops {clash} and {i} [{start},{end}) overlap inside one "
                "run(): their order is undefined")
        if end > any_end:
            any_end, any_idx = end, i
        if stores and end > store_end:
            store_end, store_idx = end, i


class ByteModel:
    def __init__(self, size, block_size=512):
        self.size = size
        self.block_size = block_size
        self.data = bytearray(size)
        self.ops_checked = 0
        self.tiles_checked = 0

    def valid(self, op):
        if op[0] == "flush":
            return True
        start, end = op_range(op)
        length = end - start
        return (length > 0 and start % self.block_size == 0
                and length % self.block_size == 0 and end <= self.size)

    def apply(self, ops):
        """Apply one run(); return the [(status, data-or-None)] it must
        produce. Reads return the bytes they must deliver."""
        valid_ops = [op for op in ops if self.valid(op)]
        assert_disjoint(valid_ops)
        expected = []
        for op in ops:
            if not self.valid(op):
                expected.append((STATUS_INVALID, None))
                continue
            kind = op[0]
            if kind == "read":
                expected.append(
                    (STATUS_OK, bytes(self.data[op[1]:op[1] + op[2]])))
                continue
            if kind == "write":
                self.data[op[1]:op[1] + len(op[2])] = op[2]
            elif kind == "fill":
                self.data[op[1]:op[1] + op[2]] = bytes([op[3] & 0xFF]) * op[2]
            expected.append((STATUS_OK, None))
        return expected

    def check(self, ops, results):
        """Apply the run and compare an engine's results with it,
        byte-exact. Raises AssertionError naming the first difference."""
        expected = self.apply(ops)
        assert len(results) == len(expected), (len(results), len(expected))
        for i, (op, want, got) in enumerate(zip(ops, expected, results)):
            label = f"op {i} {op[0]} {op[1:2]} len={op_length(op)}"
            assert got[0] == want[0], (
                f"{label}: status {got[0]}, expected {want[0]}")
            if want[1] is None:
                assert got[1] is None, f"{label}: unexpected data"
                continue
            assert got[1] is not None, f"{label}: no data returned"
            if got[1] != want[1]:
                assert len(got[1]) == len(want[1]), (
                    f"{label}: {len(got[1])} bytes, expected {len(want[1])}")
                bad = next(k for k in range(len(want[1]))
                           if got[1][k] != want[1][k])
                raise AssertionError(
                    f"{label}: first mismatch at byte {bad} (bdev offset "
                    f"{op[1] + bad}): got {got[1][bad]:#04x}, expected "
                    f"{want[1][bad]:#04x}")
        self.ops_checked += len(ops)
        self.tiles_checked += sum(op_tiles(op) for op in ops
                                  if self.valid(op))


def readback(ops):
    """Reads of exactly the ranges the run's writes and fills named."""
    return [("read", op[1], op_length(op)) for op in ops
            if op[0] in ("write", "fill")]


def guard_reads(ops, block_size=512):
    """Reads of the one block on each side of every written range."""
    out = []
    for op in ops:
        if op[0] not in ("write", "fill"):
            continue
        start, end = op_range(op)
        out.append(("read", start - block_size, block_size))
        out.append(("read", end, block_size))
    return out


class OpGenerator:
    """Seeded source of runs with pairwise-disjoint ranges.

    [lo, hi) is cut into 4 KiB-aligned slots; an op sits at
    ``slot + 4096 + 512`` — block-aligned but not tile-aligned — and
    never reaches the slot's last tile, so the block before and the
    block after every op belong to no op of any run from this
    generator (they stay at whatever the model holds there).

    Slots are handed out once (``fresh``), so ops from different calls
    never collide unless the caller asks for an old slot again with
    ``at=`` (an overwrite in a LATER run).
    """

    FILL_VALUES = (0x00, 0xFF, 0xA5, 0x3C, 0x01, 0x80)

    def __init__(self, size, seed, lengths=EDGE_LENGTHS, lo=0, hi=None):
        self.rng = random.Random(seed)
        self.lengths = tuple(lengths)
        hi = size if hi is None else hi
        self.lead = TILE + 512
        need = self.lead + max(self.lengths) + TILE
        self.stride = -(-need // TILE) * TILE
        first = -(-lo // TILE) * TILE
        self.free = list(range(first, hi - self.stride + 1, self.stride))
        self.rng.shuffle(self.free)

    def payload(self, length):
        return self.rng.randbytes(length)

    def make(self, kind, length, at=None, value=None):
        """One op of `kind` and `length` on a fresh slot, or at the
        offset `at` of an earlier op."""
        if length > max(self.lengths):
            raise ValueError("length exceeds the slot size")
        if at is None:
            if not self.free:
                raise ValueError("out of fresh slots")
            at = self.free.pop() + self.lead
        if kind == "write":
            return ("write", at, self.payload(length))
        if kind == "fill":
            if value is None:
                value = self.rng.choice(self.FILL_VALUES)
            return ("fill", at, length, value)
        if kind == "read":
            return ("read", at, length)
        raise ValueError(kind)

    def batch(self, count, kinds=("write", "fill"), lengths=None):
        """`count` ops on fresh slots. Lengths cycle through `lengths`
        (every edge is hit once per len(lengths) ops) and kinds through
        `kinds`, kind changing once per full cycle of lengths so each
        kind meets each length."""
        lengths = self.lengths if lengths is None else tuple(lengths)
        return [self.make(kinds[(i // len(lengths)) % len(kinds)],
                          lengths[i % len(lengths)])
                for i in range(count)]


# ---------------------------------------------------------------------------
# Scenarios shared by the CPU and the GPU suites. `q` is an hs.IoQueue
# on a bdev of model.size bytes that holds exactly model.data.
# ---------------------------------------------------------------------------

def run_checked(q, model, ops):
    results = q.run(ops)
    model.check(ops, results)
    return results


class RecordingQueue:
    """An hs.IoQueue that keeps the ops of every run() it passes on, so
    a test can state conditions on what a scenario actually submitted
    (which replica its reads were routed to, say)."""

    def __init__(self, queue):
        self.queue = queue
        self.runs = []

    @property
    def kind(self):
        return self.queue.kind

    def run(self, ops):
        self.runs.append(list(ops))
        return self.queue.run(ops)


def replicas_read(runs, model, n_replicas, region=1 << 20):
    """Replicas that served at least one valid read of `runs`: a
    replicated bdev routes a read to replica (offset // region) % n."""
    return {(op[1] // region) % n_replicas
            for ops in runs for op in ops
            if op[0] == "read" and model.valid(op)}


def stripe_layout(data, n_children, stripe):
    """The bytes each child of a striped bdev must hold when the bdev
    holds `data`: child c holds, in ascending order, the stripe units u
    (unit u is data[u * stripe:(u + 1) * stripe]) with u % n == c."""
    assert len(data) % (n_children * stripe) == 0
    units = [bytes(data[at:at + stripe])
             for at in range(0, len(data), stripe)]
    return [b"".join(units[child::n_children])
            for child in range(n_children)]


def scenario_tile_edges(q, model, seed):
    """Writes, fills and reads at every edge length in ONE run, at
    offsets that are block- but not tile-aligned; then read everything
    back together with the block on each side of every written range."""
    gen = OpGenerator(model.size, seed)
    n = len(EDGE_LENGTHS)
    seeded = gen.batch(n, kinds=("write",))
    run_checked(q, model, seeded)
    # Non-zero background under the fills: a fill that stops short
    # must not be masked by the zero-initialised bdev.
    under = gen.batch(n, kinds=("write",))
    run_checked(q, model, under)
    mixed = gen.batch(n, kinds=("write",))
    mixed += [gen.make("fill", op_length(op), at=op[1]) for op in under]
    mixed += [("read", op[1], op_length(op)) for op in seeded]
    mixed.append(gen.make("fill", 512, value=0x5A))
    tiles = sum(op_tiles(op) for op in mixed)
    # Odd op count above 4 and a tile count that is no multiple of the
    # batched kernel's 4 waves per workgroup: more than one workgroup
    # and a partial last one.
    assert len(mixed) % 2 == 1 and len(mixed) > 4
    assert tiles > 4 and tiles % 4 != 0
    run_checked(q, model, mixed)
    run_checked(q, model, readback(mixed) + guard_reads(mixed))
    return tiles


def scenario_mixed_batch(q, model, seed):
    """One run holding reads of earlier data, writes, fills (0x00 and
    0xFF over non-zero data among them), a flush and three requests the
    engine must reject on the host: a read crossing the end of the
    bdev, a length that is no multiple of the block size, and a
    zero-length write."""
    gen = OpGenerator(model.size, seed)
    earlier = gen.batch(5, kinds=("write",),
                        lengths=(4096, 1536, 8192 + 512, 512, 4608))
    under = gen.batch(3, kinds=("write",), lengths=(4608, 3584, 65536 + 1536))
    run_checked(q, model, earlier + under)

    odd_target = gen.make("read", 512)      # slot the 100-byte write names
    zero_target = gen.make("read", 512)
    ops = [("read", op[1], op_length(op)) for op in earlier[:3]]
    ops += gen.batch(4, kinds=("write",), lengths=(512, 4096, 3584, 8192 + 512))
    ops.append(gen.make("fill", op_length(under[0]), at=under[0][1], value=0x00))
    ops.append(("flush",))
    ops.append(("read", model.size - 512, 1024))          # crosses the end
    ops.append(gen.make("fill", op_length(under[1]), at=under[1][1], value=0xFF))
    ops.append(("write", odd_target[1], gen.payload(100)))  # not block-sized
    ops.append(gen.make("fill", op_length(under[2]), at=under[2][1], value=0xA5))
    ops.append(("write", zero_target[1], b""))            # zero length
    ops += [("read", op[1], op_length(op)) for op in earlier[3:]]
    ops.append(gen.make("fill", 1024, value=0x01))
    invalid = {i for i, op in enumerate(ops)
               if op[0] != "flush" and (op_length(op) % 512 != 0
                                        or op_length(op) == 0
                                        or op[1] + op_length(op) > model.size)}
    assert len(invalid) == 3
    results = run_checked(q, model, ops)
    for i, (status, _) in enumerate(results):
        assert status == (STATUS_INVALID if i in invalid else STATUS_OK), (
            i, ops[i][0], status)
    # Everything the run wrote, its neighbours, and the slots the two
    # rejected writes pointed at (must be untouched).
    accepted = [op for i, op in enumerate(ops) if i not in invalid]
    run_checked(q, model, readback(accepted) + guard_reads(accepted)
                + [odd_target, zero_target])
    return sum(op_tiles(op) for op in accepted)


def stripe_boundary_shapes(size, stripe, n_children, seed):
    """[(offset, length)] placed relative to stripe boundaries.

    The bdev is cut into zones of (2n + 4) stripe units. Zone 0 and the
    last zone stay free for the end cases; up to four zones in between
    (the first, the last and two seeded picks) each hold
      * one block on each side of one boundary,
      * exactly one unit,
      * n + 2 pieces with ragged ends: every child, one of them twice.
    The shapes of one zone do not touch (the first ends at or before
    the unit the second starts with, the third starts half a unit or
    more after it), and the third ends inside its zone."""
    zone = (2 * n_children + 4) * stripe
    middle = list(range(1, size // zone - 1))
    assert middle, (
        f"{size} bytes hold {size // zone} zones of {zone}: need three")
    if len(middle) > 4:
        inner = random.Random(seed).sample(middle[1:-1], 2)
        middle = sorted([middle[0], middle[-1]] + inner)
    shapes = []
    for index in middle:
        z = index * zone
        shapes.append((z + stripe - 512, 1024))
        shapes.append((z + 2 * stripe, stripe))
        shapes.append((z + 4 * stripe - 512, n_children * stripe + 1024))
        assert shapes[-1][0] + shapes[-1][1] <= z + zone
    return shapes


def scenario_stripe_boundaries(q, model, seed, stripe, n_children):
    """Writes, fills and reads cut at stripe boundaries of a striped
    bdev of `n_children` children (see stripe_boundary_shapes), the
    first block of the bdev, and a request that ends on its last byte.
    Every run holds all shapes, so the pieces of many parent requests
    sit in the children's queues together."""
    rng = random.Random(seed)
    size = model.size
    shapes = stripe_boundary_shapes(size, stripe, n_children, seed)
    seeded = [("write", at, rng.randbytes(length)) for at, length in shapes]
    run_checked(q, model, seeded)
    run_checked(q, model, readback(seeded))

    # Fills first and third: with a single zone both 0x00 and 0xFF are
    # still used, and from two zones on every shape meets both kinds.
    values = (0x00, 0xFF, 0xA5, 0x3C)
    over = []
    for i, (at, length) in enumerate(shapes):
        if i % 2 == 0:
            over.append(("fill", at, length, values[(i // 2) % len(values)]))
        else:
            over.append(("write", at, rng.randbytes(length)))
    assert {0x00, 0xFF} <= {op[3] for op in over if op[0] == "fill"}
    # End cases (zone 0 and the last zone are otherwise unused; the
    # background there is zero, so neither stores zeros).
    first = ("fill", 0, 512, 0x5A)
    last = ("write", size - stripe - 512, rng.randbytes(stripe + 512))
    over.insert(len(over) // 2, ("flush",))
    over += [first, last]
    run_checked(q, model, over)

    crossing = ("read", size - 512, 1024)
    final = readback(over) + guard_reads(over[:-2])
    # The end cases have no block before, or after, them.
    final += [("read", 512, 512), ("read", last[1] - 512, 512), crossing]
    results = run_checked(q, model, final)
    assert results[-1] == (STATUS_INVALID, None)
    return sum(op_tiles(op) for op in over)
