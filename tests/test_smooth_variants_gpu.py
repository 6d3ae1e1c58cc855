"""The smooth dynamics and the integrator of the kernels at model constants no shipped model takes (model_variants.SMOOTH_CASES):
kinematics, com_crb_mass and smooth_forces (csrc/rsr_device.hpp), integrate, implicit_integration and the need_force path of solve
(csrc/rsr_solver.hpp), discrete_acc (csrc/physics/rsr_inverse.hpp) and the lane records that feed them, against the CPU oracle, which
reads the raw arrays of the same blob.  For every (variant, family): dynamics() and actuator_force; the forward pass, one substep
and n_frames substeps in the loop of test_physics_gpu.test_physics_oracle_parity; and on the integrator variants
inverse(discrete=True).

States: model_variants.smooth_device_states: random_states(envdef, kind, 256, 11) of the shipped model, model_variants.offsets and
smooth_offsets (ctrl outside the control range in every third env).  DR off, but: euler_damped zeroes dof_damping in the odd envs
through the batch's per-env leaf (both sides of the wave-uniform eulerdamp decision run in one batch), and actuators_dr runs under
the Go2 randomisation; the oracle gets the same leaves through per-env blobs (model_variants.per_env_blobs).

The reference, the error, the rule (p99 <= 1e-5 or <= 3 x the f32 oracle's p99; every env within max(1e-4, 20 x the f32 oracle's
max)) and the exclusion of envs whose counts flip (at most 2 %): tests/physics_support.py; kinematic fields within 1e-5; no bound
here is new.  That the reference itself is right at these constants, that the states reach the branches (both ends of the ctrl
clamp, the force and actuator-force clamps on and off, both sides of the eulerdamp decision) and that every variant moves the
dynamics away from the shipped model's: tests/test_smooth_variants.py, on the CPU.

Which row of the table in tests/test_smooth_variants.py a case reaches on the device:
  Euler with eulerdamp on (the ballot of implicit_integration)   euler_damped x 4, actuators cube, smooth_combined x 2.  On the Airbot
                                                                 the damped side of the ballot is the same solve as the shipped
                                                                 implicitfast, so its output cannot tell the two apart: what tells
                                                                 is the odd, undamped envs of euler_damped beside them in one batch
  integrate's ARROW branch with a damped diagonal, need_force    euler_damped go2flat / footstand, implicitfast x 3, smooth_combined go2flat
  the explicit path on the ROWTREE / ROWCHOL kernels             euler_plain x 2, the odd envs of euler_damped cube / tshape
  discrete_acc on a Go2 model                                    the inverse test of the six cases above on Go2 families
  gear, bias0, bias2, the clamps' off sides                      actuators x 2 (lane records on the Airbot, dx_bias on the Go2)
  the rd_frc.y clamp on the Go2 kernels                          actuators go2flat, actuators_dr, smooth_combined go2flat
  per-env gainprm / biasprm leaves with bias2 != 0               actuators_dr
  grav0, grav1                                                   gravity x 3; armature on free dofs, rd_masks.w: armature x 3

Findings.  (1) implicitfast here (kernels and oracle alike) solves (M + h D) and leaves out the actuators' velocity derivative
that MuJoCo's implicitfast adds to it; with bias2 != 0 that is a different integrator, and the model was accepted.  It is refused
now (model.check_velocity_gains), and every case with bias2 runs Euler, which takes the actuator force explicitly in MuJoCo too:
see tests/test_smooth_variants.py.  No comparison here forced a change of the kernels or the oracle.
(2) The Airbot's joint clamp on the actuator force is lifted in smooth_combined only.  Lifted without armature (`actuators` on
the cube, measured once: forward and one substep as below, but after four substeps qpos p99 1.6e-2 against the f32 oracle's
2.2e-3, qacc 2.7e-2 against 8.8e-3), the position servos amplify a one-ulp change of the input qvel to 2.7e-3 of the f32 oracle's
own qpos, 20 times the shipped model's 1.2e-4, and the f32 oracle's distance is no yardstick.  `actuators` keeps the clamp at
another range (1.8e-4).  smooth_combined cube, lifted and with armature, stands at qpos 3.0e-4 / 6.8e-4 against the f32 oracle's
2.4e-4 / 8.8e-4 after four substeps: the unlimited side of rd_frc on the ROWTREE kernel agrees where rounding is not amplified.

Mutation sanity, done once by hand on the CPU-side references (a copy of the closed forms of tests/test_smooth_variants.py with one
term changed, against the f64 oracle under physics_support.rel; the rule's cap on one env is 1e-4):
  length = q, not gear q        actuator_force of actuators is off by p99 1.8 (cube), 1.5 (go2flat); least env 5.5e-2 / 6.4e-1
  bias2 x velocity dropped      actuator_force of actuators is off by p99 1.1e-2 (cube), 7.1e-3 (go2flat); median 1.4e-3 / 3.0e-3 (the
                                least env of the cube 1.4e-5: its largest forces sit on a clamp)
  grav0 = grav1 = 0             qfrc_bias at rest of gravity is off by 2.2e-1 in every env of all three families
  implicit forced to false      qvel after one step is off by p99 2.8 (euler_damped cube, its damped envs), 1.5 (euler_damped and
                                implicitfast go2flat), 1.2e-2 (smooth_combined cube, least env 3.4e-3: the armature)

Measured on an MI355X, per field p99 / max of the kernel's error against the f64 oracle, the f32 oracle's own in brackets; flips: envs left out
(kernel vs f64, f32 vs f64).  bias, passive, act: qfrc_bias, qfrc_passive, qfrc_actuator; force: actuator_force; inverse: inverse_qacc
of inverse(discrete=True) on the implicit envs (the explicit ones returned the input bit for bit in every case).
  euler_damped cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.7e-7/4.9e-7 (4.5e-7/5.2e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 1.2e-6/1.6e-6 (1.2e-6/1.6e-6); force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 1.6e-4/4.0e-4 (1.6e-4/4.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    step1    qpos 3.0e-5/1.3e-4 (3.0e-5/8.4e-5); qvel 2.2e-3/4.2e-3 (2.3e-3/4.2e-3); qacc 1.6e-4/4.0e-4 (1.6e-4/4.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    stepN    qpos 1.4e-4/1.7e-3 (2.1e-4/1.9e-3); qvel 2.5e-3/1.1e-2 (3.1e-3/1.1e-2); qacc 2.1e-3/1.6e-2 (2.1e-3/1.7e-2);
             force 4.8e-5/4.5e-4 (4.7e-5/4.4e-4)
    inverse  qacc 1.0e-5/1.2e-5 (6.2e-6/7.2e-6)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.4e-7
  euler_damped tshape
    dynamics qM 1.1e-7/1.4e-7 (1.2e-7/1.4e-7); bias 2.8e-7/3.7e-7 (3.5e-7/4.4e-7); passive 3.4e-9/3.5e-9 (3.4e-9/3.5e-9);
             act 4.6e-7/5.8e-7 (3.7e-7/1.4e-6); force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    forward  qpos 6.9e-8/9.5e-8 (7.3e-8/8.4e-8); qvel 0/0 (0/0); qacc 9.7e-5/7.3e-4 (7.5e-5/5.0e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    step1    qpos 2.9e-7/6.1e-7 (4.3e-7/6.1e-7); qvel 3.6e-3/7.1e-3 (4.8e-3/7.2e-3); qacc 7.5e-5/5.0e-4 (7.5e-5/5.0e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    stepN    qpos 2.0e-6/2.4e-5 (2.0e-6/2.3e-6); qvel 2.3e-3/6.0e-2 (1.7e-3/1.1e-2); qacc 5.2e-4/3.7e-3 (3.7e-4/3.8e-3);
             force 2.6e-7/3.4e-7 (2.7e-7/3.4e-7)
    inverse  qacc 1.7e-7/1.8e-7 (2.3e-7/2.5e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.2e-7
  euler_damped go2flat
    dynamics qM 2.2e-8/2.5e-8 (3.0e-8/3.5e-8); bias 1.3e-7/1.4e-7 (1.6e-7/1.8e-7); passive 5.6e-8/5.9e-8 (5.6e-8/5.9e-8);
             act 2.3e-7/2.5e-7 (2.6e-7/3.1e-7); force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 8.2e-6/1.1e-5 (1.2e-5/1.9e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    step1    qpos 2.1e-7/3.0e-7 (2.8e-7/4.9e-7); qvel 6.1e-6/7.4e-6 (8.4e-6/1.4e-5); qacc 4.0e-6/5.3e-6 (5.5e-6/6.0e-6);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    stepN    qpos 2.4e-5/8.4e-5 (4.5e-5/8.0e-5); qvel 3.6e-4/3.5e-3 (6.1e-4/1.8e-3); qacc 2.5e-4/3.6e-4 (1.6e-4/5.2e-4);
             force 1.8e-5/3.4e-5 (2.6e-5/1.3e-4)
    inverse  qacc 4.2e-7/4.4e-7 (3.2e-7/3.5e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  euler_damped footstand
    dynamics qM 3.7e-8/3.7e-8 (3.7e-8/3.7e-8); bias 1.1e-7/1.2e-7 (1.5e-7/1.7e-7); passive 0/0 (0/0);
             act 1.6e-7/1.7e-7 (2.3e-7/2.6e-7); force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    forward  qpos 6.0e-8/6.1e-8 (6.0e-8/6.5e-8); qvel 0/0 (0/0); qacc 3.4e-5/1.0e-4 (7.8e-5/9.7e-5);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    step1    qpos 5.0e-6/6.0e-5 (1.0e-5/1.7e-5); qvel 2.8e-5/3.8e-4 (6.5e-5/8.2e-5); qacc 2.8e-5/7.5e-5 (7.3e-5/1.0e-4);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    stepN    qpos 5.1e-2/1.9e0 (2.0e-1/2.5e0); qvel 7.4e-2/1.9e0 (2.1e-1/2.5e0); qacc 4.0e-2/3.0e0 (1.6e-1/7.1e0);
             force 5.9e-4/1.8e-3 (9.2e-4/5.1e-3)
    inverse  qacc 1.2e-7/1.2e-7 (1.2e-7/1.4e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.7e-7
  euler_plain cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.7e-7/4.9e-7 (4.5e-7/5.2e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 1.2e-6/1.6e-6 (1.2e-6/1.6e-6); force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 1.6e-4/4.0e-4 (2.0e-4/4.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    step1    qpos 3.0e-6/1.2e-5 (3.8e-6/1.2e-5); qvel 1.6e-4/4.1e-4 (2.0e-4/4.1e-4); qacc 1.6e-4/4.0e-4 (2.0e-4/4.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    stepN    qpos 2.4e-5/3.7e-4 (2.4e-5/3.7e-4); qvel 4.0e-4/1.1e-2 (3.5e-4/1.1e-2); qacc 9.7e-4/2.4e-3 (9.7e-4/2.4e-3);
             force 4.5e-6/8.3e-5 (2.7e-6/8.5e-5)
    inverse  every env explicit: the input bit for bit
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.4e-7
  euler_plain tshape
    dynamics qM 1.1e-7/1.4e-7 (1.2e-7/1.4e-7); bias 2.8e-7/3.7e-7 (3.5e-7/4.4e-7); passive 3.5e-9/5.0e-9 (3.5e-9/5.0e-9);
             act 4.6e-7/5.8e-7 (3.7e-7/1.4e-6); force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    forward  qpos 6.9e-8/9.5e-8 (7.3e-8/8.4e-8); qvel 0/0 (0/0); qacc 7.5e-5/4.5e-4 (7.5e-5/4.5e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    step1    qpos 7.0e-8/8.2e-8 (7.0e-8/8.2e-8); qvel 5.9e-5/1.2e-4 (6.0e-5/1.2e-4); qacc 7.5e-5/4.5e-4 (7.5e-5/4.5e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    stepN    qpos 1.2e-7/1.2e-7 (1.2e-7/1.2e-7); qvel 5.2e-5/8.2e-5 (5.2e-5/8.1e-5); qacc 1.3e-4/1.6e-4 (1.3e-4/1.6e-4);
             force 1.8e-7/2.5e-7 (2.2e-7/2.8e-7)
    inverse  every env explicit: the input bit for bit
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.2e-7
  implicitfast go2flat
    dynamics qM 2.2e-8/2.5e-8 (3.0e-8/3.5e-8); bias 1.3e-7/1.4e-7 (1.6e-7/1.8e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 2.3e-7/2.5e-7 (2.6e-7/3.1e-7); force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 8.2e-6/1.0e-5 (1.2e-5/1.8e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    step1    qpos 2.2e-7/4.4e-7 (3.0e-7/4.9e-7); qvel 9.2e-6/1.3e-5 (1.2e-5/1.4e-5); qacc 4.2e-6/5.0e-6 (5.5e-6/6.1e-6);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    stepN    qpos 5.3e-5/1.1e-4 (4.5e-5/8.0e-5); qvel 6.0e-4/3.5e-3 (6.1e-4/1.8e-3); qacc 2.5e-4/3.6e-4 (1.9e-4/5.2e-4);
             force 2.3e-5/3.7e-5 (3.3e-5/1.3e-4)
    inverse  qacc 4.1e-7/4.4e-7 (3.3e-7/4.8e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  implicitfast go2rough
    dynamics qM 2.3e-8/2.5e-8 (3.0e-8/3.5e-8); bias 1.3e-7/1.4e-7 (1.6e-7/1.8e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 2.3e-7/2.5e-7 (2.6e-7/3.1e-7); force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 1.6e-6/1.1e-5 (2.8e-6/1.3e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    step1    qpos 6.5e-8/1.1e-7 (6.4e-8/9.5e-7); qvel 1.8e-6/1.0e-5 (1.9e-6/6.3e-5); qacc 9.3e-7/1.0e-5 (1.1e-6/1.3e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    stepN    qpos 8.0e-7/3.2e-6 (1.8e-6/1.5e-5); qvel 2.5e-5/5.6e-5 (7.7e-5/6.5e-4); qacc 3.1e-5/3.5e-5 (7.0e-5/2.2e-3);
             force 1.1e-6/6.0e-6 (1.9e-6/1.7e-5)
    inverse  qacc 3.9e-7/4.0e-7 (3.3e-7/4.0e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  implicitfast footstand
    dynamics qM 3.7e-8/3.7e-8 (3.7e-8/3.7e-8); bias 1.1e-7/1.2e-7 (1.5e-7/1.7e-7); passive 0/0 (0/0);
             act 1.6e-7/1.7e-7 (2.3e-7/2.6e-7); force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    forward  qpos 6.0e-8/6.1e-8 (6.0e-8/6.5e-8); qvel 0/0 (0/0); qacc 3.4e-5/1.0e-4 (6.4e-5/9.7e-5);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    step1    qpos 8.5e-6/6.0e-5 (1.4e-5/2.2e-5); qvel 3.6e-5/3.8e-4 (5.2e-5/7.0e-5); qacc 2.8e-5/7.5e-5 (6.8e-5/1.0e-4);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    stepN    qpos 1.5e-1/1.9e0 (2.9e-1/2.5e0); qvel 1.4e-1/1.9e0 (2.8e-1/2.5e0); qacc 9.0e-2/3.0e0 (2.0e-1/7.1e0);
             force 1.6e-3/5.9e-3 (4.0e-3/1.5e-2)
    inverse  qacc 1.2e-7/1.7e-7 (1.3e-7/1.4e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.7e-7
  actuators cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.7e-7/4.9e-7 (4.5e-7/5.2e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 2.0e-7/1.5e-6 (2.0e-7/1.5e-6); force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 3.9e-4/5.0e-3 (3.9e-4/5.1e-3);
             force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    step1    qpos 7.0e-5/2.0e-4 (6.2e-5/2.6e-4); qvel 4.3e-3/6.4e-3 (5.2e-3/6.4e-3); qacc 3.9e-4/5.0e-3 (3.9e-4/5.1e-3);
             force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    stepN    qpos 3.4e-4/1.6e-3 (6.7e-4/2.2e-3); qvel 6.7e-3/1.6e-2 (9.2e-3/1.9e-2); qacc 6.1e-3/3.4e-2 (5.9e-3/3.7e-2);
             force 3.8e-5/2.4e-4 (1.7e-4/3.3e-4)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.4e-7
  actuators go2flat
    dynamics qM 2.2e-8/2.5e-8 (3.0e-8/3.5e-8); bias 1.3e-7/1.4e-7 (1.6e-7/1.8e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 1.4e-6/1.5e-6 (1.8e-6/2.0e-6); force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 6.8e-6/8.1e-6 (1.0e-5/1.6e-5);
             force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    step1    qpos 6.4e-8/6.7e-8 (6.2e-8/6.6e-8); qvel 3.9e-6/4.8e-6 (3.6e-6/9.2e-6); qacc 3.7e-6/4.9e-6 (3.7e-6/9.5e-6);
             force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    stepN    qpos 2.3e-7/3.5e-7 (2.3e-7/2.8e-7); qvel 9.8e-6/1.6e-5 (1.2e-5/2.1e-5); qacc 2.7e-5/3.0e-5 (4.0e-5/5.5e-5);
             force 4.1e-7/6.9e-7 (3.5e-7/5.4e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  actuators_dr go2flat
    dynamics qM 1.1e-7/1.4e-7 (1.0e-7/1.1e-7); bias 1.2e-7/1.5e-7 (1.4e-7/1.7e-7); passive 5.4e-8/5.7e-8 (5.4e-8/5.7e-8);
             act 1.3e-6/1.6e-6 (1.7e-6/2.2e-6); force 9.8e-8/1.3e-7 (1.1e-7/1.4e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 7.5e-6/1.5e-5 (6.4e-6/6.6e-6);
             force 9.8e-8/1.3e-7 (1.1e-7/1.4e-7)
    step1    qpos 6.2e-8/6.6e-8 (6.1e-8/7.3e-8); qvel 3.9e-6/6.3e-6 (4.2e-6/5.1e-6); qacc 3.9e-6/5.5e-6 (4.5e-6/6.6e-6);
             force 9.8e-8/1.3e-7 (1.1e-7/1.4e-7)
    stepN    qpos 2.4e-7/3.7e-7 (3.5e-7/5.2e-7); qvel 1.2e-5/2.7e-5 (1.9e-5/2.5e-5); qacc 2.8e-5/6.0e-5 (4.5e-5/7.2e-5);
             force 3.1e-7/7.4e-7 (4.3e-7/8.2e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.8e-7
  gravity cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.0e-7/4.3e-7 (4.4e-7/5.3e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 1.2e-6/1.6e-6 (1.2e-6/1.6e-6); force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 1.6e-4/1.0e-3 (1.9e-4/1.0e-3);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    step1    qpos 5.0e-5/1.5e-4 (4.1e-5/1.1e-4); qvel 3.0e-3/3.1e-2 (3.2e-3/3.1e-2); qacc 1.6e-4/1.0e-3 (1.9e-4/1.0e-3);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    stepN    qpos 2.4e-4/5.7e-3 (4.8e-4/5.8e-3); qvel 2.7e-3/5.7e-2 (4.2e-3/5.2e-2); qacc 6.1e-3/1.1e-1 (6.5e-3/9.9e-2);
             force 7.1e-5/4.4e-4 (8.0e-5/3.8e-4)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 1 (1, 1); kinematic fields of the forward pass <= 2.4e-7
  gravity go2flat
    dynamics qM 2.2e-8/2.5e-8 (3.0e-8/3.5e-8); bias 1.5e-7/1.5e-7 (1.5e-7/1.5e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 2.3e-7/2.5e-7 (2.6e-7/3.1e-7); force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 7.9e-6/9.0e-6 (1.2e-5/1.9e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    step1    qpos 6.4e-8/1.1e-7 (8.0e-8/1.1e-7); qvel 4.2e-6/5.0e-6 (5.4e-6/5.9e-6); qacc 4.2e-6/5.3e-6 (5.2e-6/5.9e-6);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    stepN    qpos 4.4e-7/5.4e-7 (5.1e-7/5.7e-7); qvel 7.6e-6/1.1e-5 (9.7e-6/1.3e-5); qacc 1.5e-5/2.2e-5 (1.6e-5/2.2e-5);
             force 1.1e-6/1.3e-6 (1.3e-6/2.0e-6)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  gravity footstand
    dynamics qM 3.7e-8/3.7e-8 (3.7e-8/3.7e-8); bias 1.0e-7/1.1e-7 (1.6e-7/1.8e-7); passive 0/0 (0/0);
             act 1.6e-7/1.7e-7 (2.3e-7/2.6e-7); force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    forward  qpos 6.0e-8/6.1e-8 (6.0e-8/6.5e-8); qvel 0/0 (0/0); qacc 3.4e-5/1.7e-4 (7.2e-5/1.0e-4);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    step1    qpos 9.6e-7/3.3e-6 (2.7e-6/3.5e-6); qvel 2.9e-5/9.8e-5 (7.3e-5/1.1e-4); qacc 2.9e-5/9.7e-5 (7.2e-5/1.0e-4);
             force 1.6e-7/1.7e-7 (2.3e-7/2.6e-7)
    stepN    qpos 7.3e-6/1.2e-5 (1.5e-5/2.6e-5); qvel 2.1e-5/5.6e-5 (7.2e-5/1.1e-4); qacc 6.2e-5/1.1e-4 (1.2e-4/1.4e-4);
             force 1.5e-5/2.6e-5 (2.8e-5/4.6e-5)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.7e-7
  armature cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.7e-7/4.9e-7 (4.5e-7/5.2e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 1.2e-6/1.6e-6 (1.2e-6/1.6e-6); force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 1.7e-4/3.0e-4 (1.7e-4/3.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    step1    qpos 3.4e-6/9.2e-6 (4.1e-6/1.0e-5); qvel 5.1e-4/2.2e-3 (3.2e-4/2.7e-3); qacc 1.7e-4/3.0e-4 (1.7e-4/3.0e-4);
             force 1.5e-7/1.9e-7 (1.5e-7/1.9e-7)
    stepN    qpos 7.8e-5/1.8e-4 (6.7e-5/6.4e-4); qvel 8.4e-4/1.5e-3 (6.0e-4/3.6e-3); qacc 1.7e-3/6.5e-3 (1.1e-3/4.7e-3);
             force 1.2e-4/6.4e-4 (8.5e-5/5.7e-4)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.4e-7
  armature tshape
    dynamics qM 1.1e-7/1.4e-7 (1.2e-7/1.5e-7); bias 2.8e-7/3.7e-7 (3.5e-7/4.4e-7); passive 3.5e-9/5.0e-9 (3.5e-9/5.0e-9);
             act 4.6e-7/5.8e-7 (3.7e-7/1.4e-6); force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    forward  qpos 6.9e-8/9.5e-8 (7.3e-8/8.4e-8); qvel 0/0 (0/0); qacc 1.9e-4/3.3e-4 (1.9e-4/3.3e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    step1    qpos 7.1e-8/2.1e-7 (6.8e-8/8.7e-8); qvel 1.5e-4/1.3e-3 (1.0e-4/6.6e-4); qacc 2.4e-4/6.5e-4 (2.4e-4/6.5e-4);
             force 9.6e-8/1.0e-7 (1.4e-7/1.9e-7)
    stepN    qpos 4.1e-7/1.1e-6 (2.6e-7/1.1e-6); qvel 9.0e-4/6.9e-3 (4.5e-4/6.9e-3); qacc 3.1e-4/1.4e-3 (3.2e-4/1.4e-3);
             force 2.3e-7/2.9e-7 (2.0e-7/3.3e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.2e-7
  armature go2flat
    dynamics qM 3.7e-8/3.7e-8 (3.7e-8/3.7e-8); bias 1.3e-7/1.4e-7 (1.6e-7/1.8e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 2.3e-7/2.5e-7 (2.6e-7/3.1e-7); force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 3.0e-6/4.7e-6 (3.8e-6/1.4e-5);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    step1    qpos 6.2e-8/6.5e-8 (6.6e-8/7.4e-8); qvel 1.9e-6/2.3e-6 (2.9e-6/3.7e-6); qacc 2.0e-6/2.5e-6 (3.0e-6/4.2e-6);
             force 2.3e-7/2.5e-7 (2.6e-7/3.1e-7)
    stepN    qpos 1.2e-7/1.7e-7 (1.2e-7/3.3e-7); qvel 2.4e-6/4.9e-6 (2.4e-6/9.3e-6); qacc 1.0e-5/1.8e-5 (9.5e-6/3.3e-5);
             force 4.1e-7/6.0e-7 (4.1e-7/6.1e-7)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7
  smooth_combined cube
    dynamics qM 1.4e-7/1.7e-7 (1.5e-7/1.6e-7); bias 4.0e-7/4.3e-7 (4.4e-7/5.3e-7); passive 3.5e-9/4.9e-9 (3.5e-9/4.9e-9);
             act 1.3e-7/2.1e-7 (1.3e-7/2.1e-7); force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    forward  qpos 8.2e-8/8.9e-8 (7.3e-8/8.2e-8); qvel 0/0 (0/0); qacc 2.6e-5/5.2e-5 (2.6e-5/5.1e-5);
             force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    step1    qpos 1.1e-5/5.0e-5 (1.2e-5/5.3e-5); qvel 9.4e-5/5.9e-4 (1.2e-4/6.3e-4); qacc 2.6e-5/5.2e-5 (2.6e-5/5.1e-5);
             force 1.1e-7/1.5e-7 (1.1e-7/1.5e-7)
    stepN    qpos 3.0e-4/6.8e-4 (2.4e-4/8.8e-4); qvel 7.0e-4/3.2e-3 (7.1e-4/3.6e-3); qacc 1.8e-3/1.5e-2 (1.4e-3/1.6e-2);
             force 1.4e-4/7.8e-4 (1.8e-4/8.0e-4)
    inverse  qacc 5.2e-8/5.4e-8 (5.2e-8/5.5e-8)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 2.4e-7
  smooth_combined go2flat
    dynamics qM 3.7e-8/3.7e-8 (3.7e-8/3.7e-8); bias 1.5e-7/1.5e-7 (1.5e-7/1.5e-7); passive 5.8e-8/5.9e-8 (5.8e-8/5.9e-8);
             act 1.4e-6/1.5e-6 (1.8e-6/2.0e-6); force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    forward  qpos 5.9e-8/6.1e-8 (5.5e-8/6.0e-8); qvel 0/0 (0/0); qacc 4.1e-6/4.8e-6 (5.4e-6/6.6e-6);
             force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    step1    qpos 6.4e-8/6.5e-8 (6.3e-8/6.5e-8); qvel 4.2e-6/6.3e-6 (6.2e-6/7.6e-6); qacc 4.5e-6/5.0e-6 (4.8e-6/6.4e-6);
             force 1.0e-7/1.3e-7 (1.4e-7/1.7e-7)
    stepN    qpos 1.8e-6/4.8e-6 (2.5e-6/9.4e-6); qvel 3.0e-4/1.6e-3 (5.2e-4/3.1e-3); qacc 3.4e-4/5.3e-4 (3.5e-4/6.6e-4);
             force 1.9e-6/2.8e-6 (2.8e-6/4.1e-6)
    inverse  qacc 7.8e-8/9.2e-8 (6.8e-8/7.8e-8)
    flips    forward 0 (0, 0); step1 0 (0, 0); stepN 0 (0, 0); kinematic fields of the forward pass <= 1.6e-7"""
import numpy as np
import pytest

import model_variants as V
from physics_support import inverse_inputs, make, rel, rule
from rsr_mjx_amd import prng

N = V.N
DYN = dict(qM="M", qfrc_bias="qfrc_bias", qfrc_passive="qfrc_passive", qfrc_actuator="qfrc_actuator")


def _start(variant, kind):
    """(envdef, E, phys, blobs, which, dr, qpos, qvel, ctrl): the variant's batch with its per-env leaves, not yet in the test's
    states; the oracle's blobs of the same leaves"""
    from rsr_mjx_amd.physics import Physics
    envdef, E, _, _ = make(kind, N, False, variant)
    dr = V.smooth_dr(variant, envdef)
    if dr is not None:
        E.set_randomization(dr)
    E.reset(prng.split(prng.PRNGKey(1), N))
    assert E.blob == V.blob_of(envdef)
    blobs, which = V.per_env_blobs(E.blob, dr)
    return (envdef, E, Physics(E), blobs, which, dr) + V.smooth_device_states(envdef, kind)


def _dev(x, phys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=phys.device).contiguous()


def _to_continuous(M, a, h, damp, dt):
    """mj_discreteAcc in arithmetic dt, as tests/test_inverse_gpu.py states it: a + h M^-1 (damp * a)"""
    a = a.astype(dt)
    return (a + dt(h) * np.linalg.solve(M.astype(dt), (damp.astype(dt) * a))).astype(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.SMOOTH_CASES)
def test_dynamics_terms(oracle_mod, variant, kind):
    """qM, qfrc_bias, qfrc_passive and qfrc_actuator of dynamics() and actuator_force of the forward pass against the f64 oracle
    under the rule, no env excluded, as test_dynamics_gpu.test_dynamics_terms_match_the_oracle does on the shipped models."""
    import torch
    envdef, E, phys, blobs, which, dr, qpos, qvel, ctrl = _start(variant, kind)
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    phys.dynamics()
    torch.cuda.synchronize()
    ref = V.per_env_pass(oracle_mod, blobs, which, E.dims, qpos, qvel, ctrl)
    force = V.per_env_steps(oracle_mod, blobs, which, E.dims, qpos, qvel, ctrl, 0, ("actuator_force",))
    stack = lambda p, k: force[p][k] if k == "actuator_force" else np.stack([np.asarray(r[k], np.float64).reshape(-1) for r in ref[p]])
    np.testing.assert_array_equal(phys.qM.cpu().numpy(), phys.qM.cpu().numpy().transpose(0, 2, 1))
    fails = []
    for f, name in list(DYN.items()) + [("actuator_force", "actuator_force")]:
        h = getattr(phys, f).cpu().numpy().astype(np.float64).reshape(N, -1)
        rule(f"{variant} {kind}", f, rel(h, stack("f64", name)), rel(stack("f32", name), stack("f64", name)), fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.SMOOTH_CASES)
def test_forward_and_step(oracle_mod, variant, kind):
    """The loop of test_physics_gpu.test_physics_oracle_parity on the variant's blob: forward, one substep and n_frames substeps
    against the oracle's debug forward / step with its per-substep warm start; kinematic fields of the forward pass within 1e-5,
    qacc, qvel, qpos, actuator_force (and the kinematic fields after a step) under the rule; envs whose counts flip are counted and the count is bounded (2 %).  On the
    integrator variants this is what reaches integrate's branches no shipped model runs and the Go2 solve with need_force."""
    import torch
    envdef, E, phys, blobs, which, dr, qpos, qvel, ctrl = _start(variant, kind)
    fields = ("qpos", "qvel", "qacc", "actuator_force", "xpos", "xquat", "site_xpos")
    fails = []
    for mode, nsteps in (("forward", 0), ("step1", 1), ("stepN", phys.n_substeps)):
        phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
        if nsteps:
            phys.step(None, nsteps)
        torch.cuda.synchronize()
        hip = {f: getattr(phys, f).cpu().numpy().reshape(N, -1) for f in fields}
        assert all(np.isfinite(v).all() for v in hip.values())
        ref = V.per_env_steps(oracle_mod, blobs, which, E.dims, qpos, qvel, ctrl, nsteps, fields)
        c32, c64 = ref["f32"]["counts"], ref["f64"]["counts"]
        hip_ncon = phys.contacts()["ncon"].cpu().numpy()
        flips = (hip_ncon != c64[:, 3]) | (c32 != c64).any(1)
        print(variant, kind, mode, "count flips in %d of %d envs (kernel vs f64 %d, f32 vs f64 %d)"
              % (flips.sum(), N, (hip_ncon != c64[:, 3]).sum(), (c32 != c64).any(1).sum()))
        if flips.mean() > 0.02:
            fails.append(f"{variant} {kind} {mode}: count flips in {flips.sum()} of {N} envs")
        keep = ~flips
        for f in fields:
            err = rel(hip[f], ref["f64"][f])[keep]
            spread = rel(ref["f32"][f], ref["f64"][f])[keep]
            if f in ("xpos", "xquat", "site_xpos") and mode == "forward":
                print(variant, kind, mode, f, "max %.2e" % err.max())
                if err.max() > 1e-5:
                    fails.append(f"{variant} {kind} {mode} {f}: max {err.max():.2e}")
            else:
                rule(f"{variant} {kind}", f"{mode} {f}", err, spread, fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant,kind", V.INTEGRATOR_CASES)
def test_discrete_inverse(oracle_mod, variant, kind):
    """inverse(discrete=True) at the noisy acceleration of the inverse parity test.  Where the env integrates implicitly (the
    decision restated from the model and the env's damping): inverse_qacc against a + h solve(M64, damp a) under the rule, the
    spread the same in fp32 on the f32 oracle's M (the reference and bound of test_inverse_gpu.test_discrete_accelerations).
    Where it integrates explicitly, the zero-damping envs of euler_damped included: the input bit for bit."""
    import torch
    envdef, E, phys, blobs, which, dr, qpos, qvel, ctrl = _start(variant, kind)
    A = envdef.sys.arrays
    h = float(A["opt_timestep"][0])
    damp = np.tile(np.asarray(A["dof_damping"], np.float32)[None], (N, 1)) if dr is None else np.asarray(dr["dof_damping"], np.float32)
    implicit = np.full(N, int(A["opt_integrator"][0]) == V.INT_IMPLICITFAST)
    if int(A["opt_integrator"][0]) == V.INT_EULER and int(A["opt_disable_eulerdamp"][0]) == 0:
        implicit = (damp != 0).any(1)
    want = dict(euler_damped=N // 2, euler_plain=0, implicitfast=N, smooth_combined=N)[variant]
    assert implicit.sum() == want
    phys.set_state(qpos=qpos, qvel=qvel, ctrl=ctrl)
    ref = V.per_env_pass(oracle_mod, blobs, which, E.dims, qpos, qvel, ctrl)
    a = inverse_inputs(ref["f64"], V.SEED)["noisy"]
    phys.inverse(_dev(a, phys), discrete=True)
    torch.cuda.synchronize()
    got = phys.inverse_qacc.cpu().numpy()
    ex = ~implicit
    assert (got[ex].view(np.int32) == a[ex].view(np.int32)).all(), f"{variant} {kind}: explicit envs changed"
    if implicit.any():
        ids = np.nonzero(implicit)[0]
        c64 = np.stack([_to_continuous(ref["f64"][e]["M"], a[e], h, damp[e], np.float64) for e in ids])
        c32 = np.stack([_to_continuous(ref["f32"][e]["M"], a[e], h, damp[e], np.float32) for e in ids])
        assert np.abs(c64 - a[ids]).max() > 1e-3                   # the conversion moves the input: the test shows something
        fails = []
        rule(f"{variant} {kind}", "inverse_qacc (discrete)", rel(got[ids], c64), rel(c32, c64), fails)
        assert not fails, fails


@pytest.mark.gpu
def test_velocity_gain_leaves_are_refused_under_implicitfast():
    """set_randomization on an implicitfast batch refuses per-env gainprm / biasprm leaves with a velocity term (column 2) and
    takes the same leaves without one; on the shipped Euler Go2 model it takes both (model.check_velocity_gains)."""
    for variant, refused in (("implicitfast", True), (None, False)):
        envdef, E, _, _ = make("go2flat", 8, False, variant)
        bias = np.tile(np.asarray(envdef.sys.arrays["actuator_biasprm"], np.float32)[None], (8, 1, 1))
        E.set_randomization(dict(actuator_biasprm=bias))
        bias[5, 3, 2] = -0.5
        if refused:
            with pytest.raises(NotImplementedError, match="actuator_biasprm"):
                E.set_randomization(dict(actuator_biasprm=bias))
        else:
            E.set_randomization(dict(actuator_biasprm=bias))
