"""The marshalling of the batch methods of CloverMatrix4 and CloverMatrix8 (include/clover_batch.h), characterised without a GPU:
tests/cpp/batch_marshal_trace.cpp calls every public batch method once against tests/cpp/fake_clv_batch.c, which prints every C call's name
and scalar arguments and writes into every output a number made of that vector's inputs; the client prints what the host then sees of
every output and the copy counts.  The whole output of each build -- both roundings, page-tracked and with -DCLOVER_HIP_EXPLICIT_SYNC --
must equal, byte for byte, the trace under tests/traces/, which was recorded from the class headers as they stood before the methods
shared one layer.  A pointer in another slot, rows and cols swapped, an output that is not committed or an input mapped for writing
changes the trace; the order in which one call's inputs are mapped does not."""
import subprocess

from clover_amd.build import repo_root

ROOT = repo_root()
CPP = ROOT / "tests" / "cpp"
BUILDS = [(det, explicit) for det in (True, False) for explicit in (False, True)]
IDS = [("rounding_disabled" if det else "stochastic") + ("-explicit_sync" if explicit else "-tracked") for det, explicit in BUILDS]
FAMILIES = ["clm4_mvm", "clm4_mvm_v8", "clm8_mvm", "clm4_mvm_transposed", "clm4_mvm_v8_transposed", "clm8_mvm_transposed"]
LOOPS = ["clm4_iht_batch", "clm4_iht_v8_batch", "clm8_iht_batch"]
ENTRY_POINTS = ([f + s for f in FAMILIES for s in ("_batch", "_batch_at", "_scale_and_add_batch")]
                + [f + s for f in LOOPS for s in ("", "_one_matrix")])


def _trace(tmp_path, det, explicit):
    objs = []
    for fake in ("fake_clv.c", "fake_clv_batch.c"):
        objs.append(tmp_path / (fake[:-2] + ".o"))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-c", f"-I{ROOT / 'include'}", str(CPP / fake), "-o", str(objs[-1])], check=True)
    exe = tmp_path / f"batch_marshal_trace_{int(det)}{int(explicit)}"
    cc = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []),
                         *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}", str(CPP / "batch_marshal_trace.cpp"),
                         *map(str, objs), "-o", str(exe), "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr      # no warning under -Wall -Wextra either
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout


def test_every_build_s_trace_equals_the_recorded_one_and_the_traces_name_all_24_batched_entry_points(tmp_path):
    traces = {}
    for (det, explicit), name in zip(BUILDS, IDS):
        (tmp_path / name).mkdir()
        traces[name] = _trace(tmp_path / name, det, explicit)
        assert traces[name].endswith("done\n"), name
        assert traces[name] == (ROOT / "tests" / "traces" / f"{name}.txt").read_text(), name
    # the test cannot pass by having called nothing
    assert len(set(ENTRY_POINTS)) == 24
    called = {name: {line.split()[0] for line in trace.splitlines() if line.startswith("cl")} for name, trace in traces.items()}
    assert set(ENTRY_POINTS) <= set().union(*called.values()), set(ENTRY_POINTS) - set().union(*called.values())
    # rounding disabled: all of them (the fused and the loop calls exist there only); stochastic: the calls are given a generator
    assert set(ENTRY_POINTS) <= called["rounding_disabled-tracked"]
    assert any(" rng=set " in line for line in traces["stochastic-tracked"].splitlines() if line.startswith("clm"))
