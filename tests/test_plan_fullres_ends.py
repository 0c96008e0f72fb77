"""CPU checks of the step plan at the class-map end (plan.build_plan needs the library's host-side shape predicates only): which plans form
dec_1b's dy and BatchNorm output on load, and that no other plan changes."""
import dataclasses

import pytest

from conftest import pkg

SWITCHES = ("classmap_dy_on_load", "classmap_bn_on_load")


@pytest.fixture(scope="module")
def env():
    pkg("_build").build_library()
    return pkg("plan"), pkg("_lib").lib()


def options(plan, on, **kw):
    return plan.EngineOptions(**dict({name: on for name in SWITCHES}, **kw))


def test_bf16_mode_plans_do_not_depend_on_the_switches(env):
    plan, L = env
    for shp in ((8, 512, 512), (2, 32, 32)):
        for training, want_grad in ((True, True), (True, False), (False, False)):
            a = plan.build_plan(options(plan, True, compute_dtype="bf16"), 3, 4, *shp, training, want_grad, L)
            b = plan.build_plan(options(plan, False, compute_dtype="bf16"), 3, 4, *shp, training, want_grad, L)
            assert a.rounding_points() == b.rounding_points()
            assert {n: dataclasses.asdict(p) for n, p in a.layer.items()} == {n: dataclasses.asdict(p) for n, p in b.layer.items()}
            assert a.describe() == b.describe() and (a.cat, a.fuse_pool, a.lvl4_grad) == (b.cat, b.fuse_pool, b.lvl4_grad)


def test_eval_and_inference_plans_defer_nothing_at_the_class_map(env):
    plan, L = env
    for route in ("bf16x6", "native"):
        for training, want_grad in ((False, False), (False, True), (True, False)):
            pl = plan.build_plan(options(plan, True, fp32_matrix=route), 1, 2, 2, 64, 64, training, want_grad, L)
            off = plan.build_plan(options(plan, False, fp32_matrix=route), 1, 2, 2, 64, 64, training, want_grad, L)
            assert pl.describe() == off.describe()
            assert not any(p.dy_from_classmap or p.y_in_classmap or p.x_bn_on_load for p in pl.layer.values())
            assert pl.layer["dec_1b"].y == plan.F32 and pl.layer["logits"].dx == plan.F32


def test_fp32_training_plan_shows_the_changes_and_each_switch_alone(env):
    plan, L = env
    for c, k, shp in ((1, 2, (8, 512, 512)), (3, 6, (2, 1024, 1024)), (3, 4, (2, 32, 32))):
        pl = plan.build_plan(plan.EngineOptions(), c, k, *shp, True, True, L)             # the defaults: both on
        last, cm = pl.layer["dec_1b"], pl.layer["logits"]
        assert last.dy_from_classmap and cm.dx is None and cm.dgrad == "conv1x1"
        assert last.y_in_classmap and last.y is None and cm.x_bn_on_load
        rows = {r.split()[0]: r for r in pl.describe().splitlines()[1:] if r.split()[0] in pl.layer}
        assert " dy<-classmap" in rows["dec_1b"] and " y->classmap" in rows["dec_1b"] and "y=None" in rows["dec_1b"]
        assert " bn_on_load" in rows["logits"] and "dx=None" in rows["logits"]
        # nothing else moves: the other 21 layers are the plan with both switches off, field for field
        off = plan.build_plan(options(plan, False), c, k, *shp, True, True, L)
        assert all(dataclasses.asdict(pl.layer[n]) == dataclasses.asdict(off.layer[n]) for n in pl.layer if n not in ("dec_1b", "logits"))
        assert not any(p.dy_from_classmap or p.y_in_classmap or p.x_bn_on_load for p in off.layer.values())
        assert off.layer["dec_1b"].y == plan.F32 and off.layer["logits"].dx == plan.F32
        # (the weight-fold pairs of the fused Winograd route are counted by defer_y / x_on_load and stay 13)
        assert sum(p.defer_y for p in pl.layer.values()) == 13 and sum(p.x_on_load for p in pl.layer.values()) == 13
        one = plan.build_plan(plan.EngineOptions(classmap_bn_on_load=False), c, k, *shp, True, True, L)
        assert one.layer["dec_1b"].dy_from_classmap and one.layer["logits"].dx is None
        assert not one.layer["dec_1b"].y_in_classmap and one.layer["dec_1b"].y == plan.F32 and not one.layer["logits"].x_bn_on_load
        two = plan.build_plan(plan.EngineOptions(classmap_dy_on_load=False), c, k, *shp, True, True, L)
        assert not two.layer["dec_1b"].dy_from_classmap and two.layer["logits"].dx == plan.F32 and two.layer["dec_1b"].y_in_classmap
    # more than 8 classes: the class map keeps its data gradient and its materialised input
    many = plan.build_plan(plan.EngineOptions(), 1, 12, 2, 32, 32, True, True, L)
    assert not many.layer["dec_1b"].dy_from_classmap and not many.layer["dec_1b"].y_in_classmap and many.layer["logits"].dx == plan.F32


def test_switches_are_read_from_the_environment(env):
    plan, _ = env
    o = plan.EngineOptions.from_env({})
    assert o.classmap_dy_on_load and o.classmap_bn_on_load
    o = plan.EngineOptions.from_env({"UNET_CLASSMAP_DY_ON_LOAD": "0"})
    assert not o.classmap_dy_on_load and o.classmap_bn_on_load
    o = plan.EngineOptions.from_env({"UNET_CLASSMAP_BN_ON_LOAD": "0"})
    assert o.classmap_dy_on_load and not o.classmap_bn_on_load
    assert plan.EngineOptions().key() != o.key()
