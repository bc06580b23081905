"""Pins the summation order that csrc/fixed_sum.h defines, bit for bit, through its simplest user: ops.image_mse
(mse_partial_kernel: a grid-stride loop per lane, then block_sum; mse_finish_kernel: the workgroups' totals in block order).
Everything after the f32 loads is fp64 with contraction off, so torch float64 on the host, adding in the same order, must give the
same bits.  The other users of the header are held to their own oracles elsewhere; what this file adds is the ORDER."""
import pytest
import torch

THREADS, MAX_BLOCKS = 256, 128   # color_correct.hip

# (N, H, W, C): the smallest shapes at which the order can go wrong in each way
SHAPES = [
    (2, 37, 101, 3),    # 11211 elements: 44 workgroups, the last one ragged (203 lanes hold a value), more than one image
    (1, 109, 101, 3),   # 33027 elements > 128 * 256: the workgroup count is clamped and 259 lanes take a second pass
]


def _images(shape, seed):
    """values over three decades, so that another order of the same additions really rounds differently"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 10 ** (-3 * torch.rand(shape, generator=g))


def _emulate(a, b):
    """image_mse of f32 [N,H,W,C] in torch float64 on the host, in the kernels' order"""
    sq = a.double() - b.double()
    sq = (sq * sq).reshape(a.shape[0], -1)
    n = sq.shape[1]
    blocks = min((n + THREADS - 1) // THREADS, MAX_BLOCKS)
    stride = blocks * THREADS
    passes = (n + stride - 1) // stride
    out = []
    for img in sq:
        # element e belongs to lane e % 256 of workgroup (e // 256) % blocks, which adds its elements in increasing e.  The padding
        # stands for the lanes that have no element in the last pass: x + 0.0 == x bit for bit for the x >= 0 here.
        padded = torch.cat([img, img.new_zeros(passes * stride - n)]).reshape(passes, blocks, THREADS)
        red = torch.zeros(blocks, THREADS, dtype=torch.float64)
        for p in range(passes):
            red = red + padded[p]
        s = THREADS // 2
        while s > 0:                       # block_sum: red[t] += red[t + s] for t < s
            red = red[:, :s] + red[:, s:2 * s]
            s //= 2
        total = 0.0
        for v in red[:, 0].tolist():       # mse_finish_kernel: one lane, block order
            total += v
        out.append(total / float(n))
    return torch.tensor(out, dtype=torch.float64), sq.sum(1) / float(n)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    a, b = _images(request.param, 11), _images(request.param, 12)
    emulated, plain = _emulate(a, b)
    return a, b, emulated, plain


def test_emulated_order_differs_from_plain_sum(case):
    """without this the GPU test could pass with any order: the inputs must make the order visible in the bits"""
    _, _, emulated, plain = case
    assert bool((emulated != plain).all()), (emulated.tolist(), plain.tolist())
    assert torch.allclose(emulated, plain, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_image_mse_adds_in_the_documented_order(hip_lib, case):
    from vist3a_amd import ops
    a, b, emulated, _ = case
    got = ops.image_mse(a.cuda(), b.cuda()).cpu()
    print(f"[fixed_sum {tuple(a.shape)}] gpu {got.tolist()} emulated {emulated.tolist()}")
    assert torch.equal(got, emulated)
