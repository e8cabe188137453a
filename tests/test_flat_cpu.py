"""v_diffusion.flat on CPU tensors: the flat parameter store behind both trainer.FlatState and optim.FusedAdamW (layout, the lagging
range, torch.optim.AdamW-format state, gradient slots).  No HIP kernel is launched."""
import pickle

import pytest
import torch


def _store(**kw):
    import v_diffusion
    from v_diffusion.flat import FlatParams
    from oracle.cases import TINY
    torch.manual_seed(0)
    model = v_diffusion.UNet(**TINY["tinyA"]["cfg"])           # class-conditional: class_embed.1.{weight,bias}
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    return model, FlatParams(list(model.named_parameters()), **kw), before


def _adamw_state(model, steps):
    """a torch.optim.AdamW-format state: entry i at steps[i] with recognisable moments, no entry where steps[i] is None"""
    return {i: {"step": torch.tensor(float(s)), "exp_avg": torch.full_like(p, i + 0.5), "exp_avg_sq": torch.full_like(p, i + 0.25)}
            for i, (p, s) in enumerate(zip(model.parameters(), steps)) if s is not None}


def test_views_alias_the_buffers_and_keep_the_values():
    model, st, before = _store(extra_grad=4)
    assert st.g_all.numel() == st.numel + 4 and st.g.data_ptr() == st.g_all.data_ptr()
    for k, p in model.named_parameters():
        assert st.offsets[k] % 4 == 0
        assert p.data_ptr() == st.p.data_ptr() + 4 * st.offsets[k] and torch.equal(p.detach(), before[k]), k
        for buf in (st.p, st.g, st.m, st.v):
            assert st.view(buf, k).data_ptr() == buf.data_ptr() + 4 * st.offsets[k] and st.view(buf, k).shape == p.shape


def test_adamw_state_round_trip_with_a_lagging_group():
    model, st, _ = _store()
    names = [k for k, _ in model.named_parameters()]
    cls = [k for k in names if k.startswith("class_embed.")]
    lag = st.span(cls)
    torch.manual_seed(1)
    st.m.normal_()
    st.v.uniform_()
    state = st.adamw_state(5, lag, 3)
    assert sorted(state) == list(range(len(names)))
    for i, k in enumerate(names):
        assert float(state[i]["step"]) == (3.0 if k in cls else 5.0), k
        assert torch.equal(state[i]["exp_avg"], st.view(st.m, k)) and torch.equal(state[i]["exp_avg_sq"], st.view(st.v, k))
    m, v = st.m.clone(), st.v.clone()
    st.m.fill_(7.0)
    st.v.fill_(7.0)
    assert st.load_adamw_state(state) == (5, lag, 3)
    for k in names:
        assert torch.equal(st.view(st.m, k), st.view(m, k)) and torch.equal(st.view(st.v, k), st.view(v, k)), k
    # every parameter at one step: no lagging range; step 0 writes no entry at all (torch.optim.AdamW before its first step)
    assert st.load_adamw_state(st.adamw_state(4)) == (4, None, 4)
    assert st.adamw_state(0) == {}


def test_missing_class_embedding_entries_read_as_a_lagging_range_at_step_zero():
    model, st, _ = _store()
    names = [k for k, _ in model.named_parameters()]
    cls = [k for k in names if k.startswith("class_embed.")]
    st.m.fill_(9.0)
    steps, lag, lag_steps = st.load_adamw_state(_adamw_state(model, [None if k in cls else 7 for k in names]))
    assert (steps, lag, lag_steps) == (7, st.span(cls), 0)
    for i, k in enumerate(names):
        want = 0.0 if k in cls else i + 0.5
        assert torch.all(st.view(st.m, k) == want), k


def test_non_adjacent_missing_entries_raise():
    model, st, _ = _store()
    n = len(list(model.parameters()))
    with pytest.raises(NotImplementedError):
        st.load_adamw_state(_adamw_state(model, [None if i in (0, n - 1) else 2 for i in range(n)]))
    with pytest.raises(NotImplementedError):                    # three step counts
        st.load_adamw_state(_adamw_state(model, [1 if i == 0 else 2 if i == n - 1 else 3 for i in range(n)]))


def test_gradient_slot_is_handed_out_only_while_no_earlier_view_is_alive():
    from v_diffusion.flat import owner
    model, st, _ = _store()
    k, p = next(iter(model.named_parameters()))
    assert owner(p) == (st, k)
    a = st.grad_slot(k)
    assert a.data_ptr() == st.g.data_ptr() + 4 * st.offsets[k]
    b = st.grad_slot(k)                                          # the first view is still held: a fresh tensor
    assert b.data_ptr() != a.data_ptr()
    del a, b
    c = st.grad_slot(k)
    assert c.data_ptr() == st.g.data_ptr() + 4 * st.offsets[k]
    del c
    p.grad = torch.zeros_like(p)                                 # an accumulated .grad: a fresh tensor
    assert st.grad_slot(k).data_ptr() != st.g.data_ptr() + 4 * st.offsets[k]


def test_parameters_stay_picklable():
    model, st, _ = _store()
    pickle.dumps(list(model.parameters()))
    assert not any(hasattr(p, "_vd_flat") for p in model.parameters())
