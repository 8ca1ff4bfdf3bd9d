"""CPU-side checks of the iteration's tail: ``optim.FusedAdam`` (constructor, the torch path it takes
for CPU parameters, torch's state layout and state interchange with ``torch.optim.Adam``, LR
schedulers), the ABI of ``gnca_optim_step`` / ``gnca_pool_commit`` (struct mirrors, exports, argument
checks that return before any launch) and ``SamplePool.commit``'s argument validation and CPU path."""
import copy
import ctypes
import os
import random
import subprocess

import pytest
import torch

from graph_neural_cellular_automata_amd import _lib as L
from graph_neural_cellular_automata_amd import dp
from graph_neural_cellular_automata_amd.optim import FusedAdam
from graph_neural_cellular_automata_amd.pool import SamplePool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (5, 7), (16,)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _set_grads(params, step, skip=()):
    g = torch.Generator().manual_seed(1000 + step)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g)
        p.grad = None if i in skip else grad


# ------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True), dict(lr=torch.tensor(1e-3)),
                                dict(decoupled_weight_decay=True), dict(grad_policy="scale")],
                         ids=lambda kw: next(iter(kw)))
def test_constructor_rejects_unsupported_options(kw):
    with pytest.raises(ValueError):
        FusedAdam(_params(), **kw)


def test_unsupported_option_loaded_into_a_group_is_rejected_at_step():
    ps = _params()
    opt = FusedAdam(ps, lr=1e-3)
    opt.param_groups[0]["amsgrad"] = True
    _set_grads(ps, 0)
    with pytest.raises(ValueError):
        opt.step()


# ----------------------------------------------------------------- the torch path (CPU params)
@pytest.mark.parametrize("policy", [None, "normalize", "clip"])
def test_cpu_parameters_equal_dp_policy_plus_torch_adam_bitwise(policy):
    a, b = _params(), _params()
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1)
    fa, tb = FusedAdam(a, grad_policy=policy, **kw), torch.optim.Adam(b, **kw)
    for step in range(5):
        skip = (2,) if step in (2, 3) else ()
        _set_grads(a, step, skip)
        _set_grads(b, step, skip)
        fa.step()
        dp.POLICIES[policy or "none"](b)
        tb.step()
        for p, q in zip(a, b):
            assert torch.equal(p, q), (policy, step)
    for p, q in zip(a, b):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(fa.state[p][k], tb.state[q][k])


def test_dp_none_policy_is_a_no_op():
    ps = _params()
    _set_grads(ps, 0)
    before = [p.grad.clone() for p in ps]
    assert dp.POLICIES["none"](ps) is None
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, before))


def test_state_dict_has_torchs_layout():
    a, b = _params(), _params()
    fa, tb = FusedAdam(a, lr=1e-3, grad_policy="normalize"), torch.optim.Adam(b, lr=1e-3)
    _set_grads(a, 0, skip=(1,))
    _set_grads(b, 0, skip=(1,))
    fa.step()
    dp.normalize_gradients_(b)
    tb.step()
    sa, sb = fa.state_dict(), tb.state_dict()
    assert sorted(sa) == sorted(sb) == ["param_groups", "state"]
    assert sorted(sa["param_groups"][0]) == sorted(sb["param_groups"][0])
    assert sorted(sa["state"]) == sorted(sb["state"]) == [0, 2, 3]   # no state for the skipped tensor
    for i in sa["state"]:
        assert sorted(sa["state"][i]) == sorted(sb["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k in sa["state"][i]:
            x, y = sa["state"][i][k], sb["state"][i][k]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (i, k)
        st = sa["state"][i]["step"]
        assert st.dim() == 0 and st.dtype == torch.float32 and st.device.type == "cpu" and float(st) == 1.0


@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_interchange_with_torch_adam(direction):
    kw = dict(lr=1e-2, weight_decay=0.01)
    a, b = _params(), _params()                      # a: the run that changes class, b: torch all the way
    first = torch.optim.Adam(a, **kw) if direction == "torch_to_fused" else FusedAdam(a, **kw)
    whole = torch.optim.Adam(b, **kw)
    for step in range(3):
        _set_grads(a, step)
        _set_grads(b, step)
        first.step()
        whole.step()
    second = FusedAdam(a, **kw) if direction == "torch_to_fused" else torch.optim.Adam(a, **kw)
    second.load_state_dict(copy.deepcopy(first.state_dict()))
    for step in range(3, 6):
        _set_grads(a, step)
        _set_grads(b, step)
        second.step()
        whole.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        assert float(second.state[p]["step"]) == 6.0


def test_steplr_drives_the_learning_rate():
    ps = _params()
    opt = FusedAdam(ps, lr=1e-2, grad_policy="normalize")
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1)
    seen = []
    for step in range(5):
        _set_grads(ps, step)
        opt.step()
        sched.step()
        seen.append(opt.param_groups[0]["lr"])
    assert seen == pytest.approx([1e-2, 1e-3, 1e-3, 1e-4, 1e-4])
    before = [p.detach().clone() for p in ps]
    _set_grads(ps, 9)
    opt.step()                                       # lr 1e-4: a step of about that size, not 1e-2
    delta = max(float((p.detach() - q).abs().max()) for p, q in zip(ps, before))
    assert 0 < delta < 5e-4


# ----------------------------------------------------------------------------------- the ABI
def test_descriptor_mirrors_match_the_header(tmp_path):
    structs = [("gnca_optim_tensor", L.OptimTensor), ("gnca_optim_desc", L.OptimDesc),
               ("gnca_pool_commit_desc", L.PoolCommitDesc)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gnca.h"', 'int main(void){']
    for cname, mirror in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("max %d\\n", GNCA_OPTIM_MAX_TENSORS);')
    lines.append('printf("one %d\\n", GNCA_OPTIM_ONE_LAUNCH_MAX);')
    lines.append('printf("pol %d %d %d\\n", GNCA_OPTIM_POLICY_NONE, GNCA_OPTIM_POLICY_NORMALIZE, GNCA_OPTIM_POLICY_CLIP);')
    lines.append('printf("flg %u %u\\n", GNCA_OPTIM_SUMSQ, GNCA_OPTIM_UPDATE);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for cname, mirror in structs:
        assert int(got[cname][0]) == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert int(got[f"{cname}.{f}"][0]) == getattr(mirror, f).offset, (cname, f)
    assert int(got["max"][0]) == L.OPTIM_MAX_TENSORS == 24
    assert int(got["one"][0]) == L.OPTIM_ONE_LAUNCH_MAX
    assert [int(v) for v in got["pol"]] == [L.OPTIM_POLICY_NONE, L.OPTIM_POLICY_NORMALIZE, L.OPTIM_POLICY_CLIP]
    assert [int(v) for v in got["flg"]] == [L.OPTIM_SUMSQ, L.OPTIM_UPDATE]
    assert ctypes.sizeof(L.OptimDesc) < 4096        # the descriptor travels as a kernel argument


def test_library_exports_both_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("gnca_optim_step", "gnca_pool_commit"):
        assert name in L.EXPORTS and hasattr(lib, name)
        assert f" T {name}\n" in out
    assert lib.gnca_abi_version() == 5


def _optim_desc(n=1):
    d = L.OptimDesc()
    d.policy, d.num_tensors = L.OPTIM_POLICY_NORMALIZE, n
    d.beta1, d.beta2, d.eps, d.max_norm, d.norm_eps = 0.9, 0.999, 1e-8, 0.5, 1e-8
    for i in range(min(n, L.OPTIM_MAX_TENSORS)):
        e = d.t[i]
        e.p = e.g = e.m = e.v = 256 * (i + 1)       # never dereferenced: every case fails before a launch
        e.numel, e.lr, e.bias1, e.bias2 = 4, 1e-3, 0.1, 0.001
    return d


def test_optim_step_rejects_bad_arguments_before_any_launch(lib):
    assert lib.gnca_optim_step(None, None) == -1
    d = _optim_desc()
    d.t[0].g = None                                  # a null pointer in the table
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -1
    d = _optim_desc(L.OPTIM_MAX_TENSORS + 1)
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -1
    d = _optim_desc()
    d.num_tensors = -1
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -1
    d = _optim_desc()
    d.t[0].numel = -4
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -1
    d = _optim_desc()
    d.policy = 3
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -1
    d = _optim_desc()
    d.t[0].numel = L.OPTIM_ONE_LAUNCH_MAX + 1        # too large for the one-launch form: needs the sums' workspace
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -3
    d = _optim_desc(2)
    d.sumsq, d.sumsq_base, d.sumsq_count = 4096, 1, 2   # tensor 1 would own sumsq[2]
    assert lib.gnca_optim_step(ctypes.byref(d), None) == -3
    d = _optim_desc(0)                               # nothing to do: no launch, ok
    assert lib.gnca_optim_step(ctypes.byref(d), None) == 0


def test_pool_commit_rejects_bad_arguments_before_any_launch(lib):
    def call(B=4, elems=8, slots_n=9, n_reset=1, pool=256, slots=512, state=768, per=1024, seeds=1280, seed1=None,
             rand=None, desc=True):
        d = L.PoolCommitDesc()
        d.pool_slots, d.sample_elems, d.B, d.n_reset = slots_n, elems, B, n_reset
        return lib.gnca_pool_commit(ctypes.byref(d) if desc else None, pool, slots, state, per, seeds, seed1, rand,
                                    None)

    assert call(desc=False) == -1
    assert call(pool=None) == -1 and call(slots=None) == -1 and call(state=None) == -1
    assert call(B=0) == -1 and call(B=-2) == -1 and call(elems=-8) == -1 and call(slots_n=0) == -1
    assert call(n_reset=5) == -1 and call(n_reset=-1) == -1     # n_reset > B
    assert call(per=None) == -1 and call(seeds=None) == -1       # n_reset > 0 needs both
    assert call(n_reset=0, rand=1536) == -1 and call(n_reset=0, seed1=1536) == -1   # reseed needs both


# ------------------------------------------------------------------------- SamplePool.commit
def _seed_fn(batch_size=1):
    g = torch.zeros(batch_size, 5, 3, 7)
    g[:, 3:, 1, 3] = 1.0 + 0.01 * torch.randn(batch_size, 2)
    return g


def _pool(n=7):
    torch.manual_seed(0)
    return SamplePool(n, _seed_fn)


def test_commit_validates_its_arguments():
    pool = _pool()
    idx, batch = pool.sample(5)
    per = torch.arange(5.0)
    before = pool.states.clone()
    with pytest.raises(ValueError):
        pool.commit(idx, batch, per, n_reset=1)                          # no seed_fn
    with pytest.raises(ValueError):
        pool.commit(idx, batch, n_reset=1, seed_fn=_seed_fn)             # no per_sample
    with pytest.raises(ValueError):
        pool.commit(idx, batch, reseed=True)                             # no seed_fn
    with pytest.raises(ValueError):
        pool.commit(idx, batch[:4])                                      # batch size mismatch
    with pytest.raises(ValueError):
        pool.commit(idx, batch[:, :4])                                   # channel mismatch
    with pytest.raises(ValueError):
        pool.commit(idx, batch, per[:4], n_reset=1, seed_fn=_seed_fn)    # per_sample shape
    with pytest.raises(ValueError):
        pool.commit(idx, batch, per, n_reset=6, seed_fn=_seed_fn)        # n_reset > B
    with pytest.raises(ValueError):
        pool.commit([0, 1, 1, 2, 3], batch)                              # a repeated slot
    with pytest.raises(ValueError):
        pool.commit([0, 1, 2, 3, 7], batch)                              # a slot outside the pool
    with pytest.raises(ValueError):
        pool.commit(idx, batch, per, n_reset=1, seed_fn=lambda n: torch.zeros(n, 5, 3, 6))   # seed shape
    assert torch.equal(pool.states, before)                              # nothing above wrote the pool


@pytest.mark.parametrize("n_reset", [0, 1, 5])
@pytest.mark.parametrize("reseed", [False, True])
def test_commit_on_a_cpu_pool_equals_the_reference_sequence(n_reset, reseed):
    """The trainers' write-back (topk, randint().item(), clone, two assignments, index_copy_) on
    distinct losses, under the same seeds: the same pool and the same RNG streams afterwards."""
    a, b = _pool(), _pool()
    random.seed(3)
    idx, batch = a.sample(5)
    state = batch + torch.arange(1.0, 6.0).view(5, 1, 1, 1)
    per = torch.tensor([0.3, 0.7, 0.1, 0.9, 0.5])
    torch.manual_seed(11)
    a.commit(idx, state, per, n_reset=n_reset, seed_fn=_seed_fn, reseed=reseed)
    after_a = torch.get_rng_state()
    torch.manual_seed(11)
    worst = torch.topk(per, n_reset).indices if n_reset > 0 else None
    rand_idx = torch.randint(0, 5, (1,)).item() if reseed else None
    sfp = state.clone()
    if worst is not None:
        sfp[worst] = _seed_fn(len(worst))
    if reseed:
        sfp[rand_idx:rand_idx + 1] = _seed_fn(1)
    b.replace(idx, sfp)
    assert torch.equal(a.states, b.states)
    assert torch.equal(after_a, torch.get_rng_state())


def test_commit_ranks_nan_first_and_ties_by_lower_index():
    pool = _pool()
    idx = [4, 0, 6, 2, 5]
    state = torch.full((5, 5, 3, 7), 2.0)
    per = torch.tensor([0.9, float("nan"), 0.9, 0.1, 0.9])
    seeds = torch.arange(1.0, 4.0).view(3, 1, 1, 1).expand(3, 5, 3, 7) * 10    # seeds[r] = 10 (r + 1)
    pool.commit(idx, state, per, n_reset=3, seed_fn=lambda n: seeds[:n].clone())
    # rank 0: the NaN (b = 1, slot 0); ranks 1, 2: the 0.9s at b = 0 and b = 2 (slots 4, 6); b = 4 keeps its state
    assert [float(pool.states[s, 0, 0, 0]) for s in (0, 4, 6, 2, 5)] == [10.0, 20.0, 30.0, 2.0, 2.0]
    # two NaNs rank by lower index among themselves, both above +inf
    per = torch.tensor([float("nan"), 0.5, float("nan"), float("inf"), 0.1])
    pool.commit(idx, state, per, n_reset=3, seed_fn=lambda n: seeds[:n].clone())
    assert [float(pool.states[s, 0, 0, 0]) for s in idx] == [10.0, 2.0, 20.0, 30.0, 2.0]
