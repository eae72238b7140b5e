"""-m gpu: what the host knows about every built-in problem family, seen through the C ABI alone -- which ids exist, each family's
maxderiv and shape rule (with the texts of the refusals), its parameter count, the kincar flag and whether the structured Newton modes
apply.  Nothing heavier than plan construction on the smallest spec of each family runs here; the device is needed only because
ntg_plan_create asks for one before it validates.

The workspace sizes of WORKSPACE are integers determined by the plan (layouts of ntg_batch_workspace_bytes for hessian = 0..3, batch NB);
they were read from the library as it stood before the family facts moved into one descriptor table, and hold it to the same answers."""
import dataclasses
import re

import numpy as np
import pytest
import torch

from ntg_amd import api, configs as cf
from ntg_amd.spec import FAM_MANIP, FAM_OBSTACLE, FAM_VANDERPOL

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = -2, -4
NB = 4

VALID = {
    "kincar": cf.config_K0,
    "vanderpol": cf.config_A,
    "testfam": cf.config_T,
    "obstacle": lambda: cf.config_O(ninterv=4),
    "obstacle_field1": lambda: cf.config_OF(1, ninterv=4),
    "obstacle_field3": lambda: cf.config_OF(3, ninterv=4),
    "quadrotor": lambda: cf.config_D(ninterv=4),
    "manip": lambda: cf.config_E(ninterv=4, narms=2),
}
_plans = {}


def plan_for(name):
    if name not in _plans:
        _plans[name] = api.Plan(VALID[name](), 0)
    return _plans[name]


def _two_cars():   # four flat outputs of maxderiv 3, otherwise config_O's grid
    return cf._kincar_spec(2, 6, 3, 4, 21, 5.0, "kincar-4out-k6-l4")


def _with_maxderiv(spec, d):   # every output with maxderiv d, the linear rows resized to the new flag
    nz = d * spec.nout
    return dataclasses.replace(spec, maxderiv=[d] * spec.nout, lic=np.eye(nz), lfc=np.eye(nz), ltc=np.zeros((0, nz)))


def _refused(spec, code, text):
    with pytest.raises(api.NtgError) as e:
        api.Plan(spec, 0)
    msg = str(e.value)
    assert msg.startswith(f"libntg_amd error {code}:"), msg
    assert text in msg, msg


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_spec_builds_a_plan(name):
    assert plan_for(name).h


@pytest.mark.parametrize("family", [7, 63, 200])
def test_unknown_family_id(family):
    _refused(dataclasses.replace(cf.config_K0(), family=family), BADARG, "unknown problem family")


SHAPE_REFUSALS = {
    "kincar_nnltc1": (lambda: dataclasses.replace(cf.config_K0(), nnltc=1), "no nonlinear constraints"),
    "vanderpol_two_outputs": (lambda: dataclasses.replace(cf.config_K0(), family=FAM_VANDERPOL), "one output"),
    "testfam_nnltc3": (lambda: dataclasses.replace(cf.config_T(), nnltc=3), "1/2/1"),
    "obstacle_nnltc2": (lambda: dataclasses.replace(cf.config_O(ninterv=4), nnltc=2), "obstacle family"),
    "obstacle_four_outputs": (lambda: dataclasses.replace(_two_cars(), family=FAM_OBSTACLE, nnltc=1, tcav=[(0, 0), (1, 0)]), "obstacle family"),
    "obstacle_field_nnltc0": (lambda: cf.config_OF(0, ninterv=4), "1 to 8"),
    "obstacle_field_nnltc9": (lambda: cf.config_OF(9, ninterv=4), "1 to 8"),
    "quadrotor_nnltc3": (lambda: dataclasses.replace(cf.config_D(ninterv=4), nnltc=3), "quadrotor family"),
    "manip_four_outputs": (lambda: dataclasses.replace(_two_cars(), family=FAM_MANIP), "3 outputs per arm"),
    "manip_two_arms_nnltc3": (lambda: dataclasses.replace(cf.config_E(ninterv=4, narms=2), nnltc=3), "3 outputs per arm"),
}


@pytest.mark.parametrize("case", sorted(SHAPE_REFUSALS))
def test_shape_rule_refusal(case):
    make, text = SHAPE_REFUSALS[case]
    _refused(make(), BADARG, text)


def test_wrong_maxderiv():
    _refused(_with_maxderiv(cf.config_K0(), 4), UNSUPPORTED, "wrong maxderiv")
    _refused(_with_maxderiv(cf.config_D(ninterv=4), 3), UNSUPPORTED, "wrong maxderiv")


def test_maxderiv_is_checked_before_the_shape_rule():
    _refused(dataclasses.replace(_with_maxderiv(cf.config_D(ninterv=4), 3), nnltc=3), UNSUPPORTED, "wrong maxderiv")


@pytest.mark.parametrize("name,count", [("kincar", 0), ("vanderpol", 0), ("testfam", 0), ("obstacle", 0), ("quadrotor", 0), ("manip", 0),
                                        ("obstacle_field1", 2), ("obstacle_field3", 6)])
def test_param_count(name, count):
    assert plan_for(name).param_count == count


def test_set_params_refused_without_parameters():
    with pytest.raises(api.NtgError, match="no per-problem parameters"):
        plan_for("kincar").set_params(torch.zeros((NB, 0), dtype=torch.float64, device="cuda:0"))


def _reverse(plan):
    z = torch.ones((1, 1, 3 * plan.spec.nout), dtype=torch.float64, device="cuda:0")
    out = plan.kincar_reverse(z)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["kincar", "obstacle", "obstacle_field1"])
def test_kincar_reverse_accepted(name):
    assert _reverse(plan_for(name)).shape == (1, 1, 1, 5)


def test_kincar_reverse_refused_on_another_family():
    plan = api.Plan(cf.config_T(nout=2), 0)   # nz = 3 nout, an even number of outputs: only the family can refuse it
    with pytest.raises(api.NtgError, match=re.escape(f"error {UNSUPPORTED}:")):
        _reverse(plan)


def _workspace(plan):
    return [plan.workspace_bytes(NB, api.default_opts(hessian=h)) for h in range(4)]


@pytest.mark.parametrize("name", ["kincar", "vanderpol", "testfam"])
def test_newton_modes_act_as_hessian_1_without_coupling_blocks(name):
    w = _workspace(plan_for(name))
    assert w[1] > 0 and w[2] == w[1] and w[3] == w[1], w


# ntg_batch_workspace_bytes(NB problems) for hessian = 0, 1, 2, 3
WORKSPACE = {
    "obstacle": [509504, 509504, 11200, 41344],
    "obstacle_field3": [512192, 512192, 13888, 72256],
    "quadrotor": [1330048, 1330048, 50176, 124736],
    "manip": [1493888, 1493888, 46144, 121792],
}


@pytest.mark.parametrize("name", ["obstacle", "obstacle_field3", "quadrotor", "manip"])
def test_newton_mode_workspace(name):
    w = _workspace(plan_for(name))
    assert w == WORKSPACE[name], w
