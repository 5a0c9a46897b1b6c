"""tests/guarded.py on the CPU: a torch assignment in front of and behind a float, an int64 and a uint8 tensor is reported with exactly
those names and sides, against the fixed pattern and against the record of arm(); the payload and a store of the same bits are not."""
import numpy as np
import pytest
import torch

from tests.guarded import BEHIND, FRONT, ROWS, GuardDamage, Guarded

KINDS = {"f": (torch.float32, (5, 3), 1.5), "i": (torch.int64, (7,), 3), "b": (torch.uint8, (4, 2), 1)}


def _held(G, name):
    return next((full, lead) for n, full, lead in G.held if n == name)


def _make(G, armed):
    """A float, an int64 and a uint8 tensor, one through `empty` and two through `of`; armed: the guard rows hold valid numbers."""
    rng = np.random.default_rng(0)
    G.empty("f", KINDS["f"][1], torch.float32)
    G.of("i", rng.integers(-9, 9, KINDS["i"][1]))
    G.of("b", rng.integers(0, 2, KINDS["b"][1]), dtype=torch.uint8, spill=1 if armed else 0)
    if armed:
        for name in KINDS:  # valid numbers in the guard rows: only a record can judge them
            full, lead = _held(G, name)
            full[:lead] = 2
            full[full.shape[0] - lead:] = 2
        G.arm()


@pytest.mark.parametrize("armed", [False, True])
def test_damage_is_reported_by_name_and_side(armed):
    G = Guarded("cpu")
    _make(G, armed)
    G.check()
    assert G.damaged() == []
    for name in KINDS:  # the payload is not looked at
        full, lead = _held(G, name)
        full[lead:full.shape[0] - lead] = KINDS[name][2]
    G.check()
    cases = [("f", FRONT), ("f", BEHIND), ("i", FRONT), ("i", BEHIND), ("b", FRONT), ("b", BEHIND)]
    for name, side in cases:  # one element each, alone
        full, lead = _held(G, name)
        at = (lead - 1) if side == FRONT else (full.shape[0] - lead)
        keep = full[at].clone()
        full[at].view(-1)[0] = KINDS[name][2]
        assert G.damaged() == [(name, side)]
        with pytest.raises(GuardDamage, match=r"%s: 1 element\(s\) written %s its %d rows" % (name, side, full.shape[0] - 2 * lead)) as err:
            G.check()
        assert err.value.damaged == [(name, side)]
        full[at] = keep
        assert G.damaged() == []
    for name, side in cases:  # all six at once, the far ends of the guard rows this time
        full, lead = _held(G, name)
        full[0 if side == FRONT else full.shape[0] - 1].view(-1)[-1] = KINDS[name][2]
    assert G.damaged() == cases
    with pytest.raises(AssertionError) as err:
        G.check()
    assert err.value.damaged == cases and str(err.value).count(";") == 5


def test_of_uploads_the_payload_and_spills_into_the_back_guard():
    G = Guarded("cpu")
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    x = G.of("x", a)
    y = G.of("y", a, spill=1)
    z = G.of("z", np.arange(5), dtype=torch.int32, spill=2)
    assert x.shape == (4, 3) and np.array_equal(x.numpy(), a) and x.is_contiguous()
    assert y.shape == (3, 3) and np.array_equal(y.numpy(), a[:3]) and z.shape == (3,) and z.dtype == torch.int32
    full, lead = _held(G, "y")
    assert lead == ROWS and np.array_equal(full[lead + 3].numpy(), a[3]) and torch.isnan(full[lead + 4:]).all() and torch.isnan(full[:lead]).all()
    full, lead = _held(G, "z")
    assert lead == ROWS * 64 and full[lead + 3:lead + 5].tolist() == [3, 4]
    assert G.damaged() == [("y", BEHIND), ("z", BEHIND)], "valid numbers in a guard row are damage to the pattern: arm() first"
    G.arm()
    G.check()
    full[lead + 4] = 4  # the same bits: invisible
    G.check()
    full[lead + 4] = 5
    assert G.damaged() == [("z", BEHIND)]
    w = G.empty("w", (2,), torch.float32)  # made after arm(): judged by the pattern
    w[:] = 1.0
    assert G.damaged() == [("z", BEHIND)]
    _held(G, "w")[0][0] = 0.0
    assert G.damaged() == [("z", BEHIND), ("w", FRONT)]
