"""CPU tests of the fused update over parameter groups: the ABI surface of include/fmmt_groups.h (header == _lib.GROUPS_SIGNATURES == the built
library, argument validation in front of any launch, the group record's layout) and the host halves -- train_step.group_plan,
named_step_parameters and FusedClipAdamW.load_from over several groups."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_groups_header_signatures_and_library_agree():
    """include/fmmt_groups.h (included by fmmt.h) == _lib.GROUPS_SIGNATURES == the symbols of the built library: names, every argument's type and
    the return type, as test_guard_header_signatures_and_library_agree does; the table is disjoint from all the others"""
    from facialmmt_amd import _lib, build
    assert "adamw_groups.hip" in build.SOURCES
    assert '#include "fmmt_groups.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_groups.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.GROUPS_SIGNATURES) == ["fmmt_adamw_groups", "fmmt_adamw_groups_guarded"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "GROUPS_SIGNATURES"]
    assert len(others) >= 10
    for other in others:
        assert not set(_lib.GROUPS_SIGNATURES) & set(other)
    assert len(_lib.SIGNATURES) == 59

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.GROUPS_SIGNATURES[name]
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # the guarded entry takes the plain one's list, argument for argument
    assert _lib.GROUPS_SIGNATURES["fmmt_adamw_groups_guarded"][1] == _lib.GROUPS_SIGNATURES["fmmt_adamw_groups"][1]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in _lib.GROUPS_SIGNATURES) and "fmmt_groups.h" in text and "named_step_parameters" in text
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.GROUPS_SIGNATURES)


def test_the_group_record_is_the_headers():
    """_lib.ADAMW_GROUP_FIELDS against the struct of the header: field order, the byte offsets its comments state, 32 bytes, a 16-byte multiple"""
    from facialmmt_amd import _lib
    src = open(os.path.join(ROOT, "include", "fmmt_groups.h")).read()
    assert int(re.search(r"#define\s+FMMT_ADAMW_GROUP_BYTES\s+(\d+)", src).group(1)) == _lib.ADAMW_GROUP_BYTES == 32
    body = re.search(r"typedef struct fmmt_adamw_group \{(.*?)\} fmmt_adamw_group;", src, flags=re.S).group(1)
    header = [(m.group(1), int(m.group(2))) for m in re.finditer(r"(\w+)(?:\[\d+\])?;\s*/\* byte\s+(\d+)", body)]
    dt = np.dtype(_lib.ADAMW_GROUP_FIELDS)
    assert dt.itemsize == 32 and dt.itemsize % 16 == 0
    assert header == [(n, dt.fields[n][1]) for n in dt.names] == [("lr", 0), ("beta1", 8), ("beta2", 12), ("eps", 16), ("weight_decay", 20), ("pad", 24)]


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL comes back without a device: nothing is launched for an empty table, no group, or a NULL desc / group_of / groups / step; the
    norm is optional on the plain entry and required on the guarded one"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    p += -p % 16

    def call(fn, n_desc=1, n_blocks=1, desc=p, n_groups=1, group_of=p + 64, groups=p + 96, step=p + 68, norm=p + 72):
        return fn(n_desc, n_blocks, desc, n_groups, group_of, groups, step, norm, 1.0, 1, None)
    bad_for_both = (dict(n_groups=0), dict(n_groups=-2), dict(n_desc=0), dict(n_desc=-1), dict(n_blocks=0), dict(n_blocks=-3),
                    dict(desc=None), dict(group_of=None), dict(groups=None), dict(step=None))
    for fn in (lib.fmmt_adamw_groups, lib.fmmt_adamw_groups_guarded):
        for bad in bad_for_both:
            assert call(fn, **bad) == _lib.FMMT_EINVAL == -1, bad
        assert call(fn, groups=p + 100) == _lib.FMMT_EALIGN and call(fn, group_of=p + 66) == _lib.FMMT_EALIGN
    assert call(lib.fmmt_adamw_groups_guarded, norm=None) == _lib.FMMT_EINVAL
    assert call(lib.fmmt_adamw_groups, norm=None, n_groups=0) == _lib.FMMT_EINVAL      # (a NULL norm alone is legal there: it would launch)


def _opt(groups, **kw):
    return types.SimpleNamespace(param_groups=[dict(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, **kw), **g) for g in groups], state={})


def test_group_plan_maps_records_to_groups_in_the_order_of_params():
    from facialmmt_amd.train_step import HFAdamW, group_plan
    ps = [torch.nn.Parameter(torch.zeros(n + 1)) for n in range(6)]
    extra = ps[5]                                              # the optimizer has it, `params` has not
    opt = HFAdamW([dict(params=[ps[0], ps[2], extra], lr=1e-3, weight_decay=0.05),
                   dict(params=[ps[4], ps[1]], lr=2e-3, weight_decay=0.0),
                   dict(params=[ps[3]], lr=0.0, betas=(0.8, 0.9), eps=1e-8)])
    plan = group_plan(opt, ps[:5])
    assert plan.group_of == [0, 1, 0, 2, 1]
    assert [g["lr"] for g in plan.groups] == [1e-3, 2e-3, 0.0]
    assert [g["weight_decay"] for g in plan.groups] == [0.05, 0.0, 0.0]
    assert [g["betas"] for g in plan.groups] == [(0.9, 0.999), (0.9, 0.999), (0.8, 0.9)]
    assert [g["eps"] for g in plan.groups] == [1e-6, 1e-6, 1e-8]
    assert group_plan(opt, [ps[3], ps[1]]).group_of == [2, 1]             # another order, a subset
    lr = torch.tensor(3e-3)
    assert group_plan(_opt([dict(params=ps[:2], lr=lr), dict(params=ps[2:], lr=lr)]), ps).groups[1]["lr"] is lr     # handed through, not copied
    stray = torch.nn.Parameter(torch.zeros(2))
    with pytest.raises(ValueError, match="parameter 1 .*no parameter group"):
        group_plan(opt, [ps[0], stray])
    with pytest.raises(ValueError, match="correct_bias"):
        group_plan(_opt([dict(params=ps[:2]), dict(params=ps[2:], correct_bias=False)], correct_bias=True), ps)
    for key in ("amsgrad", "maximize"):
        with pytest.raises(ValueError, match=key):
            group_plan(_opt([dict(params=ps[:2], **{key: True}), dict(params=ps[2:])]), ps)
    with pytest.raises(ValueError):
        group_plan(types.SimpleNamespace(param_groups=[]), [])


def test_named_step_parameters_names_what_the_optimizer_steps():
    from facialmmt_amd.train_step import named_step_parameters, step_parameters
    mm = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.LayerNorm(4), torch.nn.Linear(4, 2))
    mm[2].bias.requires_grad_(False)
    named = list(named_step_parameters(mm))
    assert [n for n, _ in named] == ["0.weight", "0.bias", "1.weight", "1.bias", "2.weight"]
    assert all(a is b for (_, a), b in zip(named, step_parameters(mm))) and len(named) == len(step_parameters(mm))
    master = torch.nn.Parameter(mm[0].weight.detach().float().clone())
    masters = types.SimpleNamespace(pairs=lambda: [(mm[0].weight, master)])
    named = list(named_step_parameters(mm, masters))
    assert named[0][0] == "0.weight" and named[0][1] is master and named[1][1] is mm[0].bias
    assert all(a is b for (_, a), b in zip(named, step_parameters(mm, masters)))


def _hand_made_fused(ps, group_of, hyper):
    """a FusedClipAdamW assembled by hand (the constructor needs a device), as tests/test_step_state_cpu.py does for one group"""
    from facialmmt_amd.train_step import FusedClipAdamW
    fused = FusedClipAdamW.__new__(FusedClipAdamW)
    fused.plan = types.SimpleNamespace(group_of=group_of, groups=hyper)
    fused.keep = (ps, [None] * len(ps))
    fused.m, fused.v, fused.step = [torch.ones_like(p) for p in ps], [torch.ones_like(p) for p in ps], torch.ones(())
    return fused


def test_fused_load_from_checks_every_group_before_it_copies():
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(3)]
    h0 = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    h1 = dict(betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0)
    fused = _hand_made_fused(ps, [0, 1, 0], [dict(h0, lr=1e-3), dict(h1, lr=2e-3)])

    def state(counts=(2, 2, 2)):
        return {p: {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "step": n} for p, n in zip(ps, counts)}

    def untouched():
        return all(float(t.sum()) == 3.0 for t in fused.m + fused.v) and float(fused.step) == 1.0
    for field, value in (("eps", 1e-6), ("betas", (0.9, 0.999)), ("weight_decay", 0.01)):
        opt = types.SimpleNamespace(param_groups=[dict(h0), dict(h1, **{field: value})], state=state())
        with pytest.raises(ValueError, match=f"group 1.*`{field}`"):
            fused.load_from(opt)
        assert untouched()
    with pytest.raises(ValueError, match="group 0.*`eps`"):
        fused.load_from(types.SimpleNamespace(param_groups=[dict(h0, eps=1e-3), dict(h1)], state=state()))
    assert untouched()
    with pytest.raises(ValueError, match="counters disagree"):             # group 0 at 2, group 1 at 3: one counter serves both
        fused.load_from(types.SimpleNamespace(param_groups=[dict(h0), dict(h1)], state=state((2, 3, 2))))
    assert untouched()
    with pytest.raises(ValueError, match="counters disagree"):             # HFAdamW's layout after load_hf_state_dict: a counter per group
        fused.load_from(types.SimpleNamespace(param_groups=[dict(h0, step=torch.tensor(4.0)), dict(h1, step=torch.tensor(5.0))], state=state()))
    assert untouched()
    with pytest.raises(ValueError, match="1 parameter groups loaded"):
        fused.load_from(types.SimpleNamespace(param_groups=[dict(h0)], state=state()))
    assert untouched()
    fused.load_from(types.SimpleNamespace(param_groups=[dict(h0), dict(h1)], state=state()))
    assert all(float(t.sum()) == 0.0 for t in fused.m + fused.v) and float(fused.step) == 2.0


def test_check_optimizer_state_names_the_group_whose_hyper_parameter_differs():
    """step_state.check_optimizer_state over two groups: the second group's weight decay differs -> ValueError naming group 1 and the field"""
    from facialmmt_amd import step_state
    from facialmmt_amd.train_step import HFAdamW
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in range(3)]
    opt = HFAdamW([dict(params=ps[:2], weight_decay=0.01), dict(params=ps[2:], weight_decay=0.0)], lr=1e-3)
    sd = step_state.optimizer_state(opt, [torch.zeros(2)] * 3, [torch.zeros(2)] * 3, 3)
    step_state.check_optimizer_state(sd, opt, fused=object())
    sd["param_groups"][1]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="group 1.*`weight_decay`"):
        step_state.check_optimizer_state(sd, opt, fused=object())
