"""The public surface of the Python binding, pinned: the signature of every public method of BalanceController and of every public
function of autograd.py, the length of each docstring, and the library's export list - written out as literals, so that a change of
any of them is a change of this file.  Nothing is launched and no device is touched."""
import inspect

from quadruped_control_amd import _lib
from quadruped_control_amd import autograd
from quadruped_control_amd.balance_controller import BalanceController

# name -> (str(inspect.signature(...)), len(docstring)); a length of 0: the method has never had one
CONTROLLER_METHODS = {'from_params': ('(cls, P, **kw)', 0),
 'set_kinematics': ('(self, hip=None, links=None, tau_min=None, tau_max=None, jc_kff=None, jc_kp=None, jc_kd=None, planner_hip=None, planner_k=None, '
                    'swing_height=None)',
                    162),
 'set_gait': ('(self, t_swing, t_stance)', 102),
 'set_tuning': ('(self, **kw)', 417),
 'query_launch': ('(self, n, kin=False, warm=False)', 175),
 'close': ('(self)', 0),
 'control': ('(self, Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d, foot_map, gait_map=None)', 78),
 'control_batch': ('(self, batch, warm=None, out=None, want_active_set=False, want_iterations=False, stream=None, want_torques=False)', 555),
 'plan_batch': ('(self, batch, warm=None, out=None, want_active_set=False, want_iterations=False, stream=None, want_torques=False)', 478),
 'plan_tick': ('(self, batch, command, warm=None, out=None, want_active_set=False, want_iterations=False, stream=None)', 164),
 'tick_batch': ('(self, batch, command, warm=None, out=None, want_active_set=False, want_iterations=False, stream=None)', 789),
 'plan_plant': ('(self, state, grf_body, foot_world, dt, feet=None, stream=None)', 114),
 'plant_step': ('(self, state, grf_body, foot_world, dt, feet=None, stream=None)', 692),
 'rollout': ('(self, batch, foot_world, steps, dt, warm=True, record_every=None, stream=None, certify_every=None)', 1200),
 'plan_plant_adjoint': ("(self, state, grf_body, foot_world, dt, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'grf_bar', "
                        "'foot_world_bar'), out=None, stream=None)",
                        501),
 'plant_step_adjoint': ("(self, state, grf_body, foot_world, dt, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'grf_bar', "
                        "'foot_world_bar'), out=None, stream=None)",
                        939),
 'plant_step_autograd': ('(self, state, grf_body, foot_world, dt)', 592),
 'rollout_autograd': ('(self, batch, foot_world, steps, dt, act_tol=1e-07, warm=True, params=None)', 1541),
 'plan_leg_plant': ('(self, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, cmd_state=None, foot_world=None, '
                    'flags=None, stream=None)',
                    122),
 'leg_plant_step': ('(self, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, cmd_state=None, foot_world=None, '
                    'flags=None, stream=None)',
                    1063),
 'rollout_tick': ('(self, batch, command, steps, dt, leg_inertia, warm=True, record_every=None, stream=None, certify_every=None, lean=None)', 2469),
 'plan_leg_plant_adjoint': ("(self, state, joint_tau, dt, leg_inertia, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'joint_q_bar', "
                            "'joint_qdot_bar', 'joint_tau_bar'), stance=None, gait_phase=None, gait_duty=None, cmd_state=None, out=None, flags=None, "
                            'stream=None)',
                            509),
 'leg_plant_step_adjoint': ("(self, state, joint_tau, dt, leg_inertia, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'joint_q_bar', "
                            "'joint_qdot_bar', 'joint_tau_bar'), stance=None, gait_phase=None, gait_duty=None, cmd_state=None, out=None, flags=None, "
                            'stream=None)',
                            1473),
 'leg_plant_step_autograd': ('(self, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, flags=None)', 846),
 'rollout_tick_autograd': ('(self, batch, steps, dt, leg_inertia, act_tol=1e-07, warm=True, params=None)', 1773),
 'plan_certify': ("(self, batch, grf_body, act_tol=1e-07, primal_tol=1e-07, stat_tol=1e-08, want=('primal', 'stationarity'), summary=True, out=None, "
                  'stream=None)',
                  311),
 'certify_batch': ("(self, batch, grf_body, act_tol=1e-07, primal_tol=1e-07, stat_tol=1e-08, want=('primal', 'stationarity'), summary=True, "
                   'out=None, stream=None)',
                   769),
 'plan_sensitivity': ("(self, batch, grf_body, grf_bar, want=('adjoint', 'b_bar'), act_tol=1e-07, out=None, stream=None)", 367),
 'sensitivity_batch': ("(self, batch, grf_body, grf_bar, want=('adjoint', 'b_bar'), act_tol=1e-07, out=None, stream=None)", 1039),
 'plan_sensitivity_rotation': ("(self, batch, grf_body, grf_bar, b_bar, feet_bar, want=('Rwb_bar', 'Rwb_d_bar'), out=None, stream=None)", 380),
 'sensitivity_rotation_batch': ("(self, batch, grf_body, grf_bar, b_bar, feet_bar, want=('Rwb_bar', 'Rwb_d_bar'), out=None, stream=None)", 1044),
 'parameter_tensor': ('(self)', 502),
 'plan_sensitivity_params': ("(self, batch, grf_body, grf_bar, adjoint, want=('param_bar',), act_tol=1e-07, out=None, stream=None)", 380),
 'sensitivity_params_batch': ("(self, batch, grf_body, grf_bar, adjoint, want=('param_bar',), act_tol=1e-07, out=None, stream=None)", 1574),
 'plan_sensitivity_kinematics': ('(self, batch, grf_body=None, status=None, joint_tau_bar=None, feet_bar=None, grf_bar_in=None, joint_q_bar_in=None, '
                                 "want=('joint_q_bar',), out=None, stream=None)",
                                 463),
 'sensitivity_kinematics_batch': ('(self, batch, grf_body=None, status=None, joint_tau_bar=None, feet_bar=None, grf_bar_in=None, '
                                  "joint_q_bar_in=None, want=('joint_q_bar',), out=None, stream=None)",
                                  1533),
 'plan_sensitivity_swing': ("(self, batch, joint_tau_bar, want=('swing_pos_bar', 'swing_vel_bar', 'joint_q_bar', 'joint_qdot_bar', 'Rwb_bar', "
                            "'x_bar'), out=None, joint_q_bar_in=None, Rwb_bar_in=None, x_bar_in=None, stream=None)",
                            483),
 'sensitivity_swing_batch': ("(self, batch, joint_tau_bar, want=('swing_pos_bar', 'swing_vel_bar', 'joint_q_bar', 'joint_qdot_bar', 'Rwb_bar', "
                             "'x_bar'), out=None, joint_q_bar_in=None, Rwb_bar_in=None, x_bar_in=None, stream=None)",
                             1460),
 'plan_swing_reference': ("(self, batch, want=('swing_pos', 'swing_vel'), out=None, stream=None)", 395),
 'swing_reference_batch': ("(self, batch, want=('swing_pos', 'swing_vel'), out=None, stream=None)", 1142),
 'plan_swing_reference_adjoint': ("(self, batch, state_before, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'xdot_d_bar', "
                                  "'joint_q_bar', 'p_start_bar', 'p_final_bar'), out=None, Rwb_bar_in=None, x_bar_in=None, xdot_bar_in=None, "
                                  'w_bar_in=None, joint_q_bar_in=None, stream=None)',
                                  541),
 'swing_reference_adjoint_batch': ("(self, batch, state_before, cotangents, want=('Rwb_bar', 'x_bar', 'xdot_bar', 'w_bar', 'xdot_d_bar', "
                                   "'joint_q_bar', 'p_start_bar', 'p_final_bar'), out=None, Rwb_bar_in=None, x_bar_in=None, xdot_bar_in=None, "
                                   'w_bar_in=None, joint_q_bar_in=None, stream=None)',
                                   1348),
 'swing_reference_autograd': ('(self, batch, swing_state, p_start, p_final)', 1027),
 'plan_support_polygon': ("(self, batch, schedule, world=False, want=('com_xy',), out=None, stream=None)", 375),
 'support_polygon_batch': ("(self, batch, schedule, world=False, want=('com_xy',), out=None, stream=None)", 1251),
 'plan_support_polygon_adjoint': ("(self, batch, schedule, com_xy_bar, world=False, want=('feet_bar', 'phase_bar', 'schedule_bar'), out=None, "
                                  'feet_bar_in=None, Rwb_bar_in=None, x_bar_in=None, phase_bar_in=None, schedule_bar_in=None, stream=None)',
                                  434),
 'support_polygon_adjoint_batch': ("(self, batch, schedule, com_xy_bar, world=False, want=('feet_bar', 'phase_bar', 'schedule_bar'), out=None, "
                                   'feet_bar_in=None, Rwb_bar_in=None, x_bar_in=None, phase_bar_in=None, schedule_bar_in=None, stream=None)',
                                   995),
 'support_polygon_autograd': ('(self, batch, schedule, world=False)', 617),
 'plan_com_reference': ("(self, batch, schedule, x_d, mode='replace', gain=1.0, want=('x_d',), out=None, stream=None)", 434),
 'com_reference_batch': ("(self, batch, schedule, x_d, mode='replace', gain=1.0, want=('x_d',), out=None, stream=None)", 1046),
 'plan_com_reference_adjoint': ("(self, batch, schedule, x_d_bar, mode='replace', gain=1.0, want=('x_d_in_bar', 'feet_bar', 'phase_bar', "
                                "'schedule_bar'), out=None, feet_bar_in=None, Rwb_bar_in=None, x_bar_in=None, phase_bar_in=None, "
                                'schedule_bar_in=None, stream=None)',
                                517),
 'com_reference_adjoint_batch': ("(self, batch, schedule, x_d_bar, mode='replace', gain=1.0, want=('x_d_in_bar', 'feet_bar', 'phase_bar', "
                                 "'schedule_bar'), out=None, feet_bar_in=None, Rwb_bar_in=None, x_bar_in=None, phase_bar_in=None, "
                                 'schedule_bar_in=None, stream=None)',
                                 1243),
 'com_reference_autograd': ("(self, batch, schedule, x_d, mode='replace', gain=1.0)", 635),
 'rollout_gait_autograd': ('(self, batch, steps, dt, leg_inertia, gait_dt, act_tol=1e-07, warm=True, params=None, joint_gains=None, lean=None)',
                           2017),
 'plan_commander_step': ("(self, batch, command, want=('Rwb_d', 'x_d', 'xdot_d', 'w_d'), out=None, stream=None)", 393),
 'commander_step_batch': ("(self, batch, command, want=('Rwb_d', 'x_d', 'xdot_d', 'w_d'), out=None, stream=None)", 853),
 'plan_commander_step_adjoint': ("(self, batch, command, state_before, cotangents, want=('twist_bar', 'Vb_bar', 'Rwb_bar', 'x_bar', "
                                 "'Rwb_d_prev_bar', 'x_d_prev_bar', 'xdot_d_prev_bar', 'w_d_prev_bar'), out=None, Rwb_bar_in=None, x_bar_in=None, "
                                 'stream=None)',
                                 547),
 'commander_step_adjoint_batch': ("(self, batch, command, state_before, cotangents, want=('twist_bar', 'Vb_bar', 'Rwb_bar', 'x_bar', "
                                  "'Rwb_d_prev_bar', 'x_d_prev_bar', 'xdot_d_prev_bar', 'w_d_prev_bar'), out=None, Rwb_bar_in=None, x_bar_in=None, "
                                  'stream=None)',
                                  1293),
 'commander_step_autograd': ('(self, batch, command, desired, Vb)', 921),
 'rollout_commander_autograd': ('(self, batch, command, steps, dt, leg_inertia, gait_dt, act_tol=1e-07, warm=True, params=None, joint_gains=None, '
                                'lean=None)',
                                1864),
 'tick_autograd': ('(self, batch, act_tol=1e-07, flags=None, params=None, joint_gains=None, **control_kwargs)', 1253),
 'fused_tick_autograd': ('(self, batch, act_tol=1e-07, flags=None, params=None, **control_kwargs)', 1416),
 'control_batch_autograd': ('(self, batch, act_tol=1e-07, flags=None, params=None, **control_kwargs)', 1690),
 'control_batch_host': ('(self, batch, warm=None, want_active_set=False, want_iterations=False, want_torques=False)', 74)}
AUTOGRAD_FUNCTIONS = {'control_batch_autograd': ('(ctl, batch, act_tol=1e-07, flags=None, params=None, **control_kwargs)', 430),
 'fused_tick_autograd': ('(ctl, batch, act_tol=1e-07, flags=None, params=None, **control_kwargs)', 275),
 'tick_autograd': ('(ctl, batch, act_tol=1e-07, flags=None, params=None, joint_gains=None, **control_kwargs)', 477),
 'plant_step_autograd': ('(ctl, state, grf_body, foot_world, dt)', 207),
 'rollout_autograd': ('(ctl, batch, foot_world, steps, dt, act_tol=1e-07, warm=True, params=None)', 374),
 'leg_plant_step_autograd': ('(ctl, state, joint_tau, dt, leg_inertia, stance=None, gait_phase=None, gait_duty=None, flags=None)', 238),
 'swing_reference_autograd': ('(ctl, batch, swing_state, p_start, p_final)', 277),
 'rollout_gait_autograd': ('(ctl, batch, steps, dt, leg_inertia, gait_dt, act_tol=1e-07, warm=True, params=None, joint_gains=None, lean=None)', 344),
 'commander_step_autograd': ('(ctl, batch, command, desired, Vb)', 285),
 'rollout_commander_autograd': ('(ctl, batch, command, steps, dt, leg_inertia, gait_dt, act_tol=1e-07, warm=True, params=None, joint_gains=None, '
                                'lean=None)',
                                436),
 'rollout_tick_autograd': ('(ctl, batch, steps, dt, leg_inertia, act_tol=1e-07, warm=True, params=None)', 379),
 'support_polygon_autograd': ('(ctl, batch, schedule, world=False)', 232),
 'com_reference_autograd': ("(ctl, batch, schedule, x_d, mode='replace', gain=1.0)", 223)}
EXPORTS = ('qc_create_abi',
 'qc_destroy',
 'qc_control_batch',
 'qc_control_batch_host',
 'qc_control',
 'qc_last_error',
 'qc_kernel_name',
 'qc_abi_version',
 'qc_default_kinematics',
 'qc_set_kinematics',
 'qc_set_gait',
 'qc_swing_state_init',
 'qc_set_tuning',
 'qc_query_launch',
 'qc_check_abi',
 'qc_default_command',
 'qc_commander_state_init',
 'qc_tick_batch',
 'qc_default_plant',
 'qc_plant_step_batch',
 'qc_default_leg_plant',
 'qc_leg_plant_step_batch',
 'qc_default_certify',
 'qc_certify_batch',
 'qc_default_sensitivity',
 'qc_sensitivity_batch',
 'qc_default_sensitivity_rot',
 'qc_sensitivity_rot_batch',
 'qc_default_plant_adjoint',
 'qc_plant_step_adjoint_batch',
 'qc_default_sensitivity_param',
 'qc_sensitivity_param_batch',
 'qc_default_sensitivity_kin',
 'qc_sensitivity_kin_batch',
 'qc_default_leg_plant_adjoint',
 'qc_leg_plant_step_adjoint_batch',
 'qc_default_sensitivity_swing',
 'qc_sensitivity_swing_batch',
 'qc_default_swing_reference',
 'qc_swing_reference_batch',
 'qc_default_swing_reference_adjoint',
 'qc_swing_reference_adjoint_batch',
 'qc_default_commander_step',
 'qc_commander_step_batch',
 'qc_default_commander_step_adjoint',
 'qc_commander_step_adjoint_batch',
 'qc_default_support_polygon',
 'qc_support_polygon_batch',
 'qc_default_support_polygon_adjoint',
 'qc_support_polygon_adjoint_batch',
 'qc_default_com_reference',
 'qc_com_reference_batch',
 'qc_default_com_reference_adjoint',
 'qc_com_reference_adjoint_batch')


def _surface(functions):
    return {name: (str(inspect.signature(f)), len(f.__doc__ or "")) for name, f in functions.items()}


def _public_methods(cls):
    found = {}
    for name, v in vars(cls).items():
        f = v.__func__ if isinstance(v, (classmethod, staticmethod)) else v
        if not name.startswith("_") and inspect.isfunction(f):
            found[name] = f
    return found


def _public_functions(mod):
    return {name: f for name, f in vars(mod).items() if inspect.isfunction(f) and f.__module__ == mod.__name__ and not name.startswith("_")}


def test_binding_surface():
    methods = _surface(_public_methods(BalanceController))
    assert list(methods) == list(CONTROLLER_METHODS), "the public methods of BalanceController, in their order"
    for name, (signature, doc) in CONTROLLER_METHODS.items():
        assert methods[name][0] == signature, f"BalanceController.{name}: signature"
        assert methods[name][1] == doc and (doc == 0 or BalanceController.__dict__[name].__doc__.strip()), f"BalanceController.{name}: docstring"
    functions = _surface(_public_functions(autograd))
    assert list(functions) == list(AUTOGRAD_FUNCTIONS), "the public functions of autograd.py, in their order"
    for name, (signature, doc) in AUTOGRAD_FUNCTIONS.items():
        assert functions[name][0] == signature, f"autograd.{name}: signature"
        assert functions[name][1] == doc and doc > 0 and getattr(autograd, name).__doc__.strip(), f"autograd.{name}: docstring"
    assert tuple(_lib.EXPORTS) == EXPORTS
