"""The generic LDS trainer's instantiations (csrc/mlp_fused_impl.h launch_train_bmax) as a table of shapes.

``mlp_train_kernel<L, NT, MAXQ, BMAX, BR>`` is compiled for seven ownership classes (threads, weight blocks
per thread, rows per block) x L in {2, 3, 4} x BMAX in {4, 16}: 42 kernels.  Every row of ``TABLE`` is
supported at both batch limits and lands in the same class at both, so its 21 rows reach all 42.  The widths
are ragged on purpose: they are no multiples of 4 (r4 padding, partial 4-row blocks) and mix padded and
unpadded ``ldw``.  tests/test_lds_cases_cpu.py proves the table against the plan; the GPU tests launch it.

A plain module, not a conftest: the tests import it."""

ENV = {"DCT_MLP_KERNEL": "lds", "DCT_MLP_BLOCK": "0"}  # no wave kernel, no 3x128 block kernel
CLASSES = [(256, 1, 1), (256, 2, 1), (256, 1, 4), (256, 2, 4), (256, 4, 4), (512, 3, 4), (512, 4, 4)]
BMAXES = (4, 16)

_SHAPES = {
    2: [[3, 10, 2], [30, 30, 3], [30, 54, 6], [30, 102, 6], [30, 222, 5], [90, 166, 5], [90, 250, 5]],
    3: [[1, 10, 10, 3], [1, 26, 30, 3], [10, 34, 42, 3], [11, 74, 38, 3], [17, 98, 58, 2], [17, 138, 90, 5],
        [17, 138, 150, 2]],
    4: [[1, 10, 10, 10, 6], [1, 14, 18, 30, 3], [3, 18, 50, 18, 3], [9, 34, 58, 22, 3], [1, 42, 90, 38, 6],
        [1, 90, 130, 26, 6], [3, 34, 138, 130, 6]],
}
# (dims, class), one row per (L, class)
TABLE = [(dims, cls) for L in (2, 3, 4) for dims, cls in zip(_SHAPES[L], CLASSES)]

# (dims, bmax values, class, batch of the GPU cases or None for "the usual ones", what the row is the edge of)
EDGES = [
    ([5, 510, 2], (4, 16), (256, 2, 4), None, "nbias == 512 == 2 * threads: the bias ownership's limit"),
    ([7, 160, 160, 3], (16,), (512, 4, 4), None, "159,312 B of the 163,840 B LDS budget"),
    ([15, 40, 5], (16,), (256, 1, 1), 16, "B * D0 + B == 256 threads: the batch prefetch, exact fit"),
    ([16, 40, 5], (16,), (256, 1, 1), 16, "272 > 256 threads: the direct gather"),
    ([31, 138, 150, 2], (16,), (512, 4, 4), 16, "B * D0 + B == 512 threads: the batch prefetch, exact fit"),
    ([32, 138, 150, 2], (16,), (512, 4, 4), 16, "528 > 512 threads: the direct gather"),
]
EDGE_LDS_BYTES = {(7, 160, 160, 3): 159312}


def num_params(dims):
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def kernels():
    """(dims, bmax, class) of every table row at both batch limits: 42 distinct (L, bmax, class)."""
    return [(dims, bmax, cls) for dims, cls in TABLE for bmax in BMAXES]


def smallest_per_class():
    """The row with the fewest parameters of each ownership class, in CLASSES' order."""
    return [min((d for d, c in TABLE if c == cls), key=num_params) for cls in CLASSES]


def name(dims):
    return "x".join(str(d) for d in dims)
