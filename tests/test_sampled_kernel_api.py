"""The one kernel body of the (slot, sample) rollouts (sampled_kernel, csrc/physics/rsr_sample.hpp), by its text: what the sampled,
the parameter / closed-loop and the cost rollouts share is stated once, and what one op alone has stands under that op's
`if constexpr` switch.  The stages the switches add (overlay_leaves, feedback_ctrl, cost_stage) are headers of their own.  Host
side only; the kernels are covered by tests/test_sample_gpu.py, test_param_rollouts_gpu.py, test_feedback_gpu.py and
test_cost_rollouts_gpu.py, and that each op's instructions are those of the kernel it had to itself by tools/kernel_diff.py
(DESIGN.md 4i)."""
import os
import re

from api_support import CSRC, read as _read

STAGES = r"\b(kinematics|com_crb_mass|load_mrow|smooth_forces|\w+_factor|\w+_solve|collision|make_constraint|solve)\b"
SWITCHED = r"overlay_leaves|feedback_ctrl|cost_stage|\bacc\b|\bsw\."          # what only an op's switch may name


def _kernel():
    """rsr_sample.hpp as it is, without its comments, and the lines of sampled_kernel's definition"""
    kern = _read("physics", "rsr_sample.hpp")
    code = re.sub(r"//.*", "", kern)
    k = code[code.index("void sampled_kernel("):]
    return kern, code, k[:k.index("\n}\n")]


def _regions(k):
    """[(line, switch)]: every non-blank line of the kernel with the switch it stands under -- "SWEEP" or "COST" for the statement
    or the block of an `if constexpr (SWEEP)` / `(COST)`, "!SWEEP" for such a block's else, None outside all of them"""
    out, open_, depth = [], [], 0               # open_: (switch, depth the block was opened at), innermost last
    for ln in k.splitlines():
        s = ln.strip()
        if not s:
            continue
        m = re.match(r"if constexpr \((SWEEP|COST)\)", s)
        if s.startswith("}") and open_ and open_[-1][1] == depth - 1:          # the block closes here ...
            sw, d = open_.pop()
            if s == "} else {":                                                # ... or goes on as its else
                assert not sw.startswith("!"), ln
                open_.append(("!" + sw, d))
            out.append((s, sw if s == "}" else "!" + sw))
        elif m:
            out.append((s, m.group(1)))
            if s.endswith("{"):
                open_.append((m.group(1), depth))
        else:
            out.append((s, open_[-1][0] if open_ else None))
        depth += s.count("{") - s.count("}")
    assert not open_ and depth == 1             # (the definition's own brace: _kernel stops ahead of its closing one)
    return out


def test_one_body_holds_the_loop():
    kern, code, k = _kernel()
    # one definition, instantiated per op; the three it replaces are gone from every source
    assert len(re.findall(r"\b__global__\b", code)) == 1 and "template <class C, int WAVES, class Op, class... Ap>" in code
    assert "__launch_bounds__(64)" in code
    assert ("void sampled_kernel(const DModel* __restrict__ mp, Layout L, StepArgs a, PhysArgs p, RollArgs r, typename Op::Args x, Ap... ap)") in code
    flat = re.sub(r"\s+", " ", code)
    for op in ("struct SampleOp { using Args = int; };", "struct SweepOp { using Args = SweepArgs; };",
               "struct CostOp { struct Args { SweepArgs sw; CostArgs c; }; };"):
        assert op in flat, op                                          # each op's kernel arguments behind RollArgs, as they were
    assert "constexpr bool SWEEP = !std::is_same<Op, SampleOp>::value, COST = std::is_same<Op, CostOp>::value;" in k
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".hpp")):
                text = open(os.path.join(d, f)).read()
                assert not re.search(r"\bvoid (sample|sweep|cost)_kernel\b", text) and not re.search(r"\b(sample|sweep|cost)_kernel<", text), f
    for hdr in ("rsr_sweep.hpp", "rsr_cost.hpp", "rsr_feedback.hpp"):                     # the stages' headers hold no kernel
        assert "__global__" not in _read("physics", hdr), hdr
    # the stages every op shares are called once, not restated
    assert code.count("forward<C>(") == 1 and code.count("integrate<C>(") == 1
    for w in ("sensor_stage<C>(", "force_stage<C>(e, ", "load_overrides<C>(m, s, a, e, lane)", "lrec_lane(lane)", "if constexpr (C::XFRC)"):
        assert k.count(w) >= 1, w
    assert k.count("load_overrides<C>(") == 1 and k.count("sensor_stage<C>(") == 1 and k.count("force_stage<C>(") == 1
    for w in ("store_pipeline", "store_side", "asm", "atomic", "hipMalloc"):
        assert w not in kern, w
    named = re.findall(STAGES, code)
    assert not named, named
    for w in ("void overlay_leaves(", "void feedback_ctrl(", "void cost_stage(", "float differentiate_pos(", "float wave_sum("):
        assert w not in code, w
    # the record is read only, and neither the side buffer nor the sensordata row is written
    assert "const float* rec = a.state + (size_t)e * L.rec;" in k and not re.search(r"(?<!const )float\* rec\b", code)
    assert not re.search(r"\brec\[[^\]]*\]\s*=[^=]", code) and "p.sd" not in code and "p.out" not in code and "sw.ctrl_out" not in code
    # one flattened loop, the rows by workgroup in size_t, the six trajectory stores once each
    assert len(re.findall(r"\bfor \(int k = 0; k < total; \+\+k\)", code)) == 1 and k.count("const int total = r.T * p.nsteps;") == 1
    assert k.count("const size_t row = (size_t)b * r.T + t;") == 1
    assert "slot = b / K" in k and "p.ids ? p.ids[slot] : slot" in k and k.count("if (e < 0 || e >= a.n) return;") == 1
    assert k.count("const int lt = lrec_lane(lane);") == 1 and k.count("if (++t < r.T) {") == 1
    for out in ("qpos", "qvel", "time", "aforce", "ncon", "sd"):
        assert len(re.findall(r"\br\.%s\[row\b[^\]]*\] = " % out, k)) == 1, out
    assert sorted(set(re.findall(r"\br\.(\w+)\[[^\]]*\] = ", k))) == ["aforce", "ncon", "qpos", "qvel", "sd", "time"]


def test_what_one_op_alone_has_stands_under_its_switch():
    _, code, k = _kernel()
    lines = _regions(k)
    text = lambda *sw: "\n".join(ln for ln, r in lines if r in sw)
    # nothing outside a switch names a stage, the accumulators or a member of the sweep's arguments
    stray = [ln for ln, r in lines if r not in ("SWEEP", "COST") and re.search(SWITCHED, ln)]
    assert stray == [], stray
    assert [ln for ln, r in lines if r == "COST" and re.search(r"overlay_leaves|feedback_ctrl", ln)] == []
    assert [ln for ln, r in lines if r == "SWEEP" and re.search(r"cost_stage|\bacc\b|\bx\.c\b", ln)] == []
    shared, sweep, cost, sample = text(None), text("SWEEP"), text("COST"), text("!SWEEP")
    # outside the switches: the whole loop, and no ctrl row (each form of its two loads is an op's own)
    for w in ("forward<C>(", "integrate<C>(", "load_overrides<C>(", "sensor_stage<C>(", "for (int k = 0; k < total; ++k)", "r.qpos[row * C::NQ + q] = s.qpos[q];",
              "if (++t < r.T) {", "const float* rec = ", "if constexpr (C::XFRC)"):
        assert shared.count(w) == 1, w
    assert "r.ctrl[" not in shared and len(re.findall(r"\bWSYNC\(\);", shared)) == 3
    # SampleOp: its two ctrl loads in its own form, and nothing else
    assert [ln for ln in sample.splitlines() if ln not in ("} else {", "}")] == ["if (lane < C::NU) s.ctrl[lane] = r.ctrl[(size_t)b * r.T * C::NU + lane];",
                                                                      "if (lt < C::NU) s.ctrl[lt] = r.ctrl[(row + 1) * C::NU + lt];"]
    # SWEEP: K, the overlay between load_overrides and forward, ctrl by slot or by workgroup in size_t, feedback_ctrl twice
    assert "if constexpr (SWEEP) K = sw.K; else K = x;" in sweep
    assert sweep.count("overlay_leaves<C>(m, s, sw, b, lane)") == 1
    assert k.index("load_overrides<C>(m, s, a, e, lane)") < k.index("overlay_leaves<C>(m, s, sw, b, lane)") < k.index("forward<C>(")
    assert "size_t cb = 0;" in shared and "if constexpr (SWEEP) cb = sw.ctrl_per_sample ? (size_t)b : (size_t)slot;" in sweep
    assert sweep.count("if (lane < C::NU) s.ctrl[lane] = r.ctrl[cb * r.T * C::NU + lane];") == 1
    assert sweep.count("if (lt < C::NU) s.ctrl[lt] = r.ctrl[(cb * r.T + t) * C::NU + lt];") == 1
    calls = [ln for ln in k.splitlines() if "feedback_ctrl<C>(" in ln]
    assert len(calls) == 2 and all(ln.strip().startswith("if (sw.fb_gain) feedback_ctrl<C>(m, hot, s, sw, ") for ln in calls)
    # the first after the first ctrl load and ahead of its fence, the second inside the boundary's `if (++t < r.T)`
    first, second = k.index(calls[0]), k.index(calls[1])
    assert k.index("s.ctrl[lane] = r.ctrl[cb") < first < k.index("const int total") and k.index("if (++t < r.T)") < k.index("s.ctrl[lt] = r.ctrl[(cb") < second
    assert "(size_t)b * r.T + t, lt);" in calls[1] and "(size_t)b * r.T, lane);" in calls[0]
    assert calls[0].count("sw.fb_per_sample ? (size_t)b : (size_t)slot") == 1 == calls[1].count("sw.fb_per_sample ? (size_t)b : (size_t)slot")
    # COST: the LDS bound, the accumulators behind Smem<C> zeroed ahead of the loop, the stage after the sensors and the
    # trajectory rows and ahead of the next ctrl row
    assert "static_assert(4 * WAVES * cost_lds_bytes<C>() <= 160 * 1024" in cost
    assert cost.count("float* acc = reinterpret_cast<float*>(smem_raw + cost_acc_offset<C>());") == 2
    assert cost.count("if (lane < 8) acc[lane] = 0.0f;") == 1 and k.index("acc[lane] = 0.0f;") < k.index("for (int k = 0;")
    assert cost.count("cost_stage<C>(hot, s, acc, x.c, (size_t)slot * r.T + t, row, (size_t)b, t == r.T - 1, lt, sv, nsd);") == 1
    assert k.index("sensor_stage<C>(") < k.index("r.sd[row * nsd + lt] = sv;") < k.index("cost_stage<C>(") < k.index("if (++t < r.T)") \
        < k.index("s.ctrl[lt] = r.ctrl[")


def test_the_overlay_is_a_stage_of_its_own():
    kern = _read("physics", "rsr_sweep.hpp")
    code = re.sub(r"//.*", "", kern)
    assert "void overlay_leaves(" in code and '#include "rsr_feedback.hpp"' in code
    for w in ("store_pipeline", "store_side", "asm", "atomic"):
        assert w not in kern, w
    # all nine images, rows in size_t, friction through the geom slots, every load ahead of the first store
    ov = code[code.index("void overlay_leaves("):]
    for img in ("s.fric[", "s.mass[", "s.damp[", "s.floss[", "s.dx_ipos[", "s.dx_qpos0[", "s.dx_arma[", "s.dx_gain[", "s.dx_bias["):
        assert ov.count(img) == 1, img
    assert "(size_t)b * width" in ov and "m.geom_slot_ids[tt / 3]" in ov and "C::NGA == C::NG" in ov and "WSYNC" not in ov
    first_store = min(m.start() for m in re.finditer(r"\bs\.\w+\[[^\]]*\] = ", ov))
    last_load = max(m.start() for m in re.finditer(r"= p_\w+\[", ov))
    assert last_load < first_store


def test_the_cost_stage_is_a_stage_of_its_own():
    kern = _read("physics", "rsr_cost.hpp")
    code = re.sub(r"//.*", "", kern)
    assert '#include "rsr_sweep.hpp"' in code and code.count("differentiate_pos<C>(") == 1
    for w in ("wave_sum(", "constexpr size_t cost_lds_bytes()", "constexpr size_t cost_acc_offset()", "#pragma clang fp contract(off)"):
        assert w in code, w
    for w in ("void overlay_leaves(", "void feedback_ctrl(", "float differentiate_pos(", "float wave_sum(", "asm", "atomic", "store_pipeline", "store_side",
              "hipMalloc", "p.sd", "p.out", "sw.ctrl_out", "forward<C>(", "integrate<C>("):
        assert w not in code, w
    assert not re.search(r"\brec\[[^\]]*\]\s*=[^=]", code)
    # the accumulators are LDS words of lane 0, not registers carried across forward<C>
    stage = code[code.index("void cost_stage("):]
    assert "if (lane == 0) acc[0] = acc[0] + ct;" in stage
    stores = set(re.findall(r"\b(c\.\w+)\[[^\]]*\] = ", stage))
    assert stores == {"c.cost", "c.step_cost", "c.terms", "c.dx", "c.ctrl_out"}, stores
