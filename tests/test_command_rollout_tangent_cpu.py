"""CPU: what rollout_commander_tangent() and rollout_lean_tangent() refuse before anything touches the device, their tables and flag
shifts, and the existing rollouts' refusals of `command` and `lean`, kept in their words."""
import pytest


class Ctl:  # never reached
    device = 0


T_ = object()
FULL = dict(joint_q=T_, joint_qdot=T_, gait_phase=T_, swing_state=T_)


def test_tables_and_flag_shifts(built):
    from quadruped_control_amd import tangent as T

    assert T.COMMANDER_FLAGS_SHIFT == 24 and T.LEAN_FLAGS_SHIFT == 25 and T.REFERENCE_FLAGS_SHIFT == 20
    assert set(T.ROLLOUT_COMMANDER_TANGENTS) == set(T.ROLLOUT_GAIT_TANGENTS) | {"twist_tan", "Vb_tan", "schedule_tan"}
    assert set(T.ROLLOUT_LEAN_TANGENTS) == set(T.ROLLOUT_GAIT_TANGENTS) | {"schedule_tan"}
    assert set(T.ROLLOUT_GAIT_TANGENTS) == set(T.ROLLOUT_TICK_TANGENTS) | {"p_start_tan", "p_final_tan"}  # (pinned elsewhere too: unchanged)


def test_the_new_rollouts_refuse_before_the_device(built):
    from quadruped_control_amd import tangent as T

    for fn, args in ((T.rollout_commander_tangent, lambda b: (Ctl(), b, {"state": T_}, 1, 0.01, 0.02, 0.01, {})),
                     (T.rollout_lean_tangent, lambda b: (Ctl(), b, 1, 0.01, 0.02, 0.01, {"schedule": T_}, {}))):
        who = fn.__name__
        for name in ("stance", "swing_pos", "swing_vel", "gait_dt", "feet"):
            with pytest.raises(ValueError, match=f"{who}: batch\\['{name}'\\] must be None"):
                fn(*args(dict(FULL, **{name: T_})))
        for name in FULL:
            with pytest.raises(ValueError, match=f"{who}: the batch carries joint_q, joint_qdot, gait_phase and swing_state - missing \\['{name}'\\]"):
                fn(*args({k: v for k, v in FULL.items() if k != name}))
    for name in ("Rwb_d", "x_d", "xdot_d", "w_d"):
        with pytest.raises(ValueError, match=f"rollout_commander_tangent: batch\\['{name}'\\] must be None - in commander mode the desired state lives"):
            T.rollout_commander_tangent(Ctl(), dict(FULL, **{name: T_}), {"state": T_}, 1, 0.01, 0.02, 0.01, {})
    with pytest.raises(ValueError, match="rollout_commander_tangent: command\\['state'\\] is required"):
        T.rollout_commander_tangent(Ctl(), FULL, {}, 1, 0.01, 0.02, 0.01, {})
    with pytest.raises(ValueError, match="rollout_commander_tangent: unknown tangent"):
        T.rollout_commander_tangent(Ctl(), FULL, {"state": T_}, 1, 0.01, 0.02, 0.01, {"swing_pos_tan": T_})
    with pytest.raises(ValueError, match="rollout_lean_tangent: lean is required"):
        T.rollout_lean_tangent(Ctl(), FULL, 1, 0.01, 0.02, 0.01, None, {})
    with pytest.raises(ValueError, match="rollout_lean_tangent: lean needs batch\\['x_d'\\]"):
        T.rollout_lean_tangent(Ctl(), FULL, 1, 0.01, 0.02, 0.01, {"schedule": T_}, {})
    with pytest.raises(ValueError, match="rollout_lean_tangent: unknown tangent"):
        T.rollout_lean_tangent(Ctl(), dict(FULL, x_d=T_), 1, 0.01, 0.02, 0.01, {"schedule": T_}, {"twist_tan": T_})


def test_the_existing_rollouts_keep_their_refusals(built):
    from quadruped_control_amd import tangent as T

    with pytest.raises(ValueError, match="rollout_gait_tangent: lean has no forward mode - lean must be None \\(the com reference has no forward mode\\)"):
        T.rollout_gait_tangent(Ctl(), FULL, 1, 0.01, 0.02, 0.01, {}, lean={})
    with pytest.raises(ValueError, match="rollout_tick_tangent: commander mode has no forward mode - command must be None \\(the desired state is held in the batch\\)"):
        T.rollout_tick_tangent(Ctl(), dict(joint_q=T_, joint_qdot=T_), 1, 0.01, 0.02, {}, command={})
    with pytest.raises(ValueError, match="rollout_swing_tangent: lean has no forward mode - lean must be None"):
        T.rollout_swing_tangent(Ctl(), dict(joint_q=T_, joint_qdot=T_, swing_pos=T_, swing_vel=T_), 1, 0.01, 0.02, {}, lean={})
