"""CPU suite: the comparison semantics and the random policies of tests/support.py, on which the GPU files rely."""
import pytest
import torch

import support


def test_same_nan_pattern_passes_by_bits_and_fails_by_value():
    for dtype in (torch.float64, torch.float32):
        a = {"k": torch.tensor([1.0, float("nan"), -2.5], dtype=dtype)}
        b = {"k": a["k"].clone()}
        support.same_dicts(a, b, ("k",))
        support.same_dicts(a, b, ("k",), by="bits")
        with pytest.raises(AssertionError):
            support.same_dicts(a, b, ("k",), by="value")


def test_signed_zeros_differ_by_bits():
    class Env:
        def __init__(self, *row):
            self.x = torch.tensor([row], dtype=torch.float32)
    support.same_env(Env(0.0, 1.0), Env(-0.0, 1.0), keys=("x",), by="value")
    support.same_env(Env(-0.0, 1.0), Env(-0.0, 1.0), keys=("x",))
    with pytest.raises(AssertionError):
        support.same_env(Env(0.0, 1.0), Env(-0.0, 1.0), keys=("x",))
    support.same_env(Env(5.0, 6.0, 7.0, 8.0), Env(6.0, 7.0), keys=("x",), sl=slice(1, 3))      # a's envs 1 .. 2 are b


def test_bits_views_floats_and_leaves_integers_alone():
    for dtype in (torch.int32, torch.int64, torch.uint8):
        t = torch.arange(6, dtype=dtype)
        assert support.bits(t) is t
    for dtype, words in ((torch.float64, torch.int64), (torch.float32, torch.int32)):
        b = support.bits(torch.tensor([1.0, -0.0], dtype=dtype))
        assert b.dtype == words and b.shape == (2,) and int(b[1]) != 0
    assert support.bits(torch.ones(4, 6, dtype=torch.float64).t()).shape == (6, 4)       # made contiguous first


def test_random_policy_repeats_for_a_seed():
    a, b, c = support.random_policy(seed=7), support.random_policy(seed=7), support.random_policy(seed=8)
    assert len(a.W) == 3 and all(torch.equal(x, y) for x, y in zip(a.W + a.b, b.W + b.b))
    assert not torch.equal(a.W[0], c.W[0])


def test_bias_gain_changes_the_biases_only():
    a, b, one = support.random_policy(gain=0.3), support.random_policy(gain=0.3, bias_gain=1.0), support.random_policy()
    assert all(torch.equal(x, y) for x, y in zip(a.W, b.W)) and not any(torch.equal(x, y) for x, y in zip(a.W, one.W))
    assert not any(torch.equal(x, y) for x, y in zip(a.b, b.b)) and all(torch.equal(x, y) for x, y in zip(b.b, one.b))
