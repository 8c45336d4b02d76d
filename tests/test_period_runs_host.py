"""CPU: how Engine.run_iterations routes runs of whole periods to step_periods (include/sactd3.h: sactd3_step_periods), and what the
entry points refuse without an engine."""
import ctypes as C
from types import SimpleNamespace

import pytest

import sac_td3_cudagraphs_pytorch_amd as P
from sac_td3_cudagraphs_pytorch_amd import _lib
from sac_td3_cudagraphs_pytorch_amd.engine import Engine


def stub(delay, td3, freq, calls, with_runs):
    s = SimpleNamespace(cfg=SimpleNamespace(actor_update_delay=delay, prefer_td3_over_sac=td3, crit_targ_update_freq=freq),
                        step=lambda a: calls.append(("step", bool(a))), step_period=lambda: calls.append(("period",)),
                        step_prefix=lambda m: calls.append(("prefix", m)))
    if with_runs:
        s.step_periods = lambda k: calls.append(("periods", k))
    return s


@pytest.mark.parametrize("delay,td3,freq", [(2, False, 1), (2, True, 1), (1, False, 1), (2, False, 2), (0, False, 1)])
def test_run_iterations_issues_two_or_more_whole_periods_as_one_call(delay, td3, freq):
    """With step_periods the launches still cover exactly iterations i0 .. i0 + n - 1 with the actor updates at the multiples of the
    period; every stretch of two or more whole periods is ONE step_periods call, a lone whole period stays a step_period call.  An
    engine object without the method gets today's sequence: the three old kinds of call only, one step_period per whole period."""
    period = delay + 1
    can = delay > 0 and (td3 or freq == 1)
    for i0 in range(0, 7):
        for n in range(0, 26):
            calls, old = [], []
            assert Engine.run_iterations(stub(delay, td3, freq, calls, True), i0, n) == i0 + n
            assert Engine.run_iterations(stub(delay, td3, freq, old, False), i0, n) == i0 + n
            assert all(c[0] in ("step", "period", "prefix") for c in old)
            i, expanded = i0, []
            for c in calls:
                if c[0] == "periods":
                    assert can and i % period == 0 and c[1] >= 2
                    i += period * c[1]
                    expanded += [("period",)] * c[1]
                elif c[0] == "period":
                    assert can and i % period == 0
                    i += period
                    expanded.append(c)
                elif c[0] == "prefix":
                    assert can and i % period == 0 and 1 <= c[1] <= delay and c is calls[-1]
                    i += c[1]
                    expanded.append(c)
                else:
                    assert c[1] == (i % period == 0)
                    i += 1
                    expanded.append(c)
            assert i == i0 + n
            assert expanded == old                                  # the same iterations in the same forms, only bundled
            whole = max(0, (i0 + n) // period - (i0 + period - 1) // period) if can else 0
            assert sum(c[0] == "periods" for c in calls) == (1 if whole >= 2 else 0)
            assert sum(c[0] == "period" for c in calls) == (1 if whole == 1 else 0)
            assert sum(c[0] == "period" for c in old) == whole


def test_entry_points_refuse_a_null_engine():
    lib = P.load_library()
    st = (C.c_int64 * 4)()
    assert lib.sactd3_step_periods(None, 2) == _lib.EINVAL
    assert lib.sactd3_step_periods_stats(None, st) == _lib.EINVAL
