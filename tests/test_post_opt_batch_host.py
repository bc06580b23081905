"""Host-side checks of batched post-optimisation and the visibility-masked Adam (no GPU): the batch order, the reference's
hyper-parameter scaling, the config's validation, the new argument struct against the header's text, and the numpy oracle of
tests/visible_adam_oracle.py against its own definition."""
import sys
from math import sqrt
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import visible_adam_oracle as VO  # noqa: E402
from c_layout import assert_mirrors  # noqa: E402


def test_batch_size_one_is_the_view_order_in_singletons():
    from vist3a_amd.post_opt import train_batch_order, train_view_order
    for n, steps, seed, k in ((5, 13, 7, 0), (7, 20, 3, 3), (1, 4, 0, 0), (6, 0, 1, 2)):
        assert train_batch_order(n, steps, seed, k, 1) == [[j] for j in train_view_order(n, steps, seed, k)]
    assert train_batch_order(5, 13, 7) == [[j] for j in train_view_order(5, 13, 7)]            # the defaults: no hold-out, one view


def test_epochs_are_cut_into_chunks_with_a_short_last_one():
    from vist3a_amd.post_opt import train_batch_order, view_order
    order = train_batch_order(5, 7, 11, 0, 3)
    assert [len(b) for b in order] == [3, 2, 3, 2, 3, 2, 3]
    flat = view_order(5, 20, 11)                                                               # the same permutations, epoch by epoch
    for e in range(3):
        a, b = order[2 * e], order[2 * e + 1]
        assert a + b == flat[5 * e:5 * e + 5]
        assert not set(a) & set(b) and sorted(a + b) == list(range(5))
    assert order[6] == flat[15:18]
    assert train_batch_order(5, 7, 11, 0, 3) == order and train_batch_order(5, 7, 12, 0, 3) != order
    assert [len(b) for b in train_batch_order(6, 4, 0, 0, 3)] == [3, 3, 3, 3]                  # B divides the views: no short batch
    assert [len(b) for b in train_batch_order(2, 3, 0, 0, 4)] == [2, 2, 2]                     # B above the views: one batch per epoch
    with pytest.raises(ValueError):
        train_batch_order(5, 3, 0, 0, 0)


def test_held_out_views_never_appear():
    from vist3a_amd.post_opt import train_batch_order, train_views
    order = train_batch_order(8, 9, 5, 3, 2)                                                   # views 0, 3, 6 held out: 5 training views
    train = train_views(8, 3)
    assert train == [1, 2, 4, 5, 7]
    assert [len(b) for b in order] == [2, 2, 1] * 3
    for e in range(3):
        epoch = sum(order[3 * e:3 * e + 3], [])
        assert sorted(epoch) == train
    g = torch.Generator().manual_seed(5)
    assert sum(order[:3], []) == [train[j] for j in torch.randperm(5, generator=g).tolist()]


@pytest.mark.parametrize("B", [1, 2, 4])
def test_hyperparameters_follow_the_reference(B):
    from vist3a_amd.post_opt import PostOptConfig, batch_hyperparameters
    cfg = PostOptConfig(batch_size=B)
    h = batch_hyperparameters(cfg)
    base = dict(means=1.6e-4, scales=5e-3, quats=1e-3, opacities=5e-2, sh=2.5e-3)
    assert set(h) == {"lr", "eps", "betas", "lr_scale"} and set(h["lr"]) == set(base)
    if B == 1:      # today's numbers, exactly: nothing multiplied, nothing divided
        assert h["lr"] == base and h["eps"] == 1e-15 and h["betas"] == (0.9, 0.999) and h["lr_scale"] == 1.0
        assert all(type(x) is float for x in (*h["lr"].values(), h["eps"], *h["betas"], h["lr_scale"]))
        return
    r = sqrt(B)
    assert h["lr"] == {n: x * r for n, x in base.items()} and h["eps"] == 1e-15 / r and h["lr_scale"] == r
    assert h["betas"] == (1 - B * (1 - 0.9), 1 - B * (1 - 0.999))
    assert h["betas"] == pytest.approx({2: (0.8, 0.998), 4: (0.6, 0.996)}[B], abs=1e-15)
    other = batch_hyperparameters(PostOptConfig(batch_size=B, lr_means=1.0, eps=1e-8, betas=(0.95, 0.99)))
    assert other["lr"]["means"] == r and other["eps"] == 1e-8 / r and other["betas"] == (1 - B * (1 - 0.95), 1 - B * (1 - 0.99))


def test_check_batch():
    from vist3a_amd.post_opt import PostOptConfig
    for B in range(1, 10):
        PostOptConfig(batch_size=B).check_batch()
        PostOptConfig(batch_size=B, visible_adam=True).check_batch()
    for bad in (0, -1, 10, 11, True, 2.0, "2", None):
        with pytest.raises(ValueError, match="batch_size"):
            PostOptConfig(batch_size=bad).check_batch()
    with pytest.raises(ValueError, match="unresolved"):                                        # says why 10 is refused
        PostOptConfig(batch_size=10).check_batch()
    with pytest.raises(ValueError, match="visible_adam"):
        PostOptConfig(visible_adam=1).check_batch()
    c = PostOptConfig()
    assert c.batch_size == 1 and c.visible_adam is False


def test_post_optimize_validates_the_batch():
    from test_post_opt_host import _gaussians
    from vist3a_amd.post_opt import PostOptConfig, post_optimize
    img, ext, K = torch.zeros(2, 16, 16, 3), torch.eye(4).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="batch_size"):
        post_optimize(_gaussians(1), img, ext, K, PostOptConfig(batch_size=10), steps=1)


def test_struct_matches_the_header():
    from vist3a_amd import lib
    assert_mirrors(lib.AdamVisibleArgs, "v3a_adam_visible_args")
    assert "v3a_adam_step_visible" in lib.SYMBOLS and "v3a_gs_visibility" in lib.SYMBOLS
    header = (Path(__file__).resolve().parents[1] / "include" / "vist3a_hip.h").read_text()
    assert f"(currently {lib.EXPECTED_ABI})" in header


def test_cli_flags_parse():
    from vist3a_amd.utils.argument import inference_vist3a_argument as get_parser
    need = ["--checkpoint_path", "c", "--transformer_lora_path", "l", "--input_texts_path", "t"]
    a = get_parser().parse_args(need)
    assert a.post_opt_batch_size == 1 and a.post_opt_visible_adam is False
    a = get_parser().parse_args(need + ["--post_opt_batch_size", "4", "--post_opt_visible_adam"])
    assert a.post_opt_batch_size == 4 and a.post_opt_visible_adam is True


def test_oracle_is_its_definition():
    """Element by element in Python floats (fp64) against the vectorised oracle; invisible rows and their NaN gradients stay out."""
    rng = np.random.default_rng(0)
    U, K = 7, 4
    p, g, m = (rng.standard_normal((U, 3, K)) for _ in range(3))
    v = rng.random((U, 3, K))
    vis = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    g[vis == 0] = np.nan
    kw = dict(lr=1e-2, lr2=5e-4, period=K, betas=(0.8, 0.998), eps=1e-15)
    pn, mn, vn = VO.adam_step_visible(p, g, m, v, vis, **kw)
    for e in range(p.size):
        i = np.unravel_index(e, p.shape)
        if not vis[i[0]]:
            assert (pn[i], mn[i], vn[i]) == (p[i], m[i], v[i])
            continue
        m1 = 0.8 * m[i] + (1 - 0.8) * g[i]
        v1 = 0.998 * v[i] + (1 - 0.998) * g[i] * g[i]
        lr = 1e-2 if e % K == 0 else 5e-4
        assert mn[i] == m1 and vn[i] == v1 and pn[i] == p[i] - lr * m1 / (np.sqrt(v1) + 1e-15)
    assert np.isfinite(pn).all() and not np.shares_memory(pn, p)
    p32 = VO.adam_step_visible(p, g, m, v, vis, dtype=np.float32, **kw)[0]
    assert p32.dtype == np.float32 and np.allclose(p32, pn, rtol=1e-5)
    r = np.array([[0, -3, 5, 0], [0, 2, -1, 0]])
    assert VO.visibility(r).tolist() == [0, 1, 1, 0] and VO.visibility(r).dtype == np.uint8
