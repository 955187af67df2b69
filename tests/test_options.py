"""The NEUS_* switches' parse rules (neus2_amd/csrc/options.h): the header alone, compiled into a
stand-alone program with the address and undefined-behaviour sanitizers, run as a child process with a constructed
environment; the program prints every field of NeusOptions::from_env(), process_options() and alloc_debug_from_env().
No GPU and no library: the header includes no HIP header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include "options.h"
#include <cstdio>
#define B(f) std::printf(#f "=%d\n", o.f ? 1 : 0);
#define I(f) std::printf(#f "=%lld\n", (long long)o.f);
int main() {
	{
		const NeusOptions o = NeusOptions::from_env();
		B(main_prio) B(lookahead) I(la_at_cut) I(la_at_full) I(la_prio) B(ev_sysfence) B(la_stat) B(adam_overlap) B(exchange_overlap)
		B(eager_ema_h) I(march_waves) I(march_lanes) B(march_balance) I(march_dbg) B(ray_cull) B(ray_sort) B(prog_cut) B(march_cut)
		I(march_cut_div) I(chunk_rounds) B(occ_sort) B(occ_nu_sort) I(scatter_mode) I(scatter_chunk) I(scatter_level_groups)
		I(scatter_xcd_group) B(scatter_noskip) B(dbg_loss_replay) B(dbg_loss_fence)
		std::printf("chunk_scale=%g\n", (double)o.chunk_scale);
		std::printf("chunk_ends=");
		for (size_t k = 0; k < o.chunk_ends.size(); ++k) std::printf(k ? ",%u" : "%u", o.chunk_ends[k]);
		std::printf("\n");
	}
	{
		const NeusProcessOptions& o = process_options();
		B(infer_xcd_parts) B(infer_pipe) I(infer_grid) I(mlp_blocks_pct)
	}
	{
		const NeusAllocDebug o = alloc_debug_from_env();
		B(log) B(poison) I(byte) I(lo)
		std::printf("hi=%llu\n", o.hi);
	}
	return 0;
}
"""

DEFAULTS = {
    "main_prio": "1", "lookahead": "1", "la_at_cut": "1", "la_at_full": "0", "la_prio": "-1", "ev_sysfence": "0", "la_stat": "0",
    "adam_overlap": "0", "exchange_overlap": "1", "eager_ema_h": "0", "march_waves": "0", "march_lanes": "8", "march_balance": "1",
    "march_dbg": "0", "ray_cull": "1", "ray_sort": "1", "prog_cut": "1", "march_cut": "1", "march_cut_div": "1", "chunk_ends": "",
    "chunk_scale": "2", "chunk_rounds": "2", "occ_sort": "1", "occ_nu_sort": "0", "scatter_mode": "2", "scatter_chunk": "512",
    "scatter_level_groups": "0", "scatter_xcd_group": "4", "scatter_noskip": "0", "dbg_loss_replay": "0", "dbg_loss_fence": "0",
    "infer_xcd_parts": "0", "infer_pipe": "1", "infer_grid": "0", "mlp_blocks_pct": "100",
    "log": "0", "poison": "0", "byte": "0", "lo": "0", "hi": str(2 ** 64 - 1),
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("options")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    exe = d / "probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "neus2_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(**env):
        # nothing of the caller's environment: no NEUS_* variable, no preload
        out = subprocess.run([str(exe)], env={"PATH": os.environ.get("PATH", "")} | env, capture_output=True, text=True, check=True).stdout
        return dict(l.split("=", 1) for l in out.splitlines())
    return run


def test_defaults(probe):
    assert probe() == DEFAULTS


@pytest.mark.parametrize("value", ["0", "1", "", "x"])
def test_switch_polarity(probe, value):
    """Only "0" turns a default-on switch off, only "1" turns a default-off switch on."""
    got = probe(NEUS_LOOKAHEAD=value, NEUS_ADAM_OVERLAP=value)
    assert got["lookahead"] == ("0" if value == "0" else "1")
    assert got["adam_overlap"] == ("1" if value == "1" else "0")
    assert {k: v for k, v in got.items() if k not in ("lookahead", "adam_overlap")} == \
           {k: v for k, v in DEFAULTS.items() if k not in ("lookahead", "adam_overlap")}


SWITCHES = {  # variable -> field
    "NEUS_MAIN_PRIO": "main_prio", "NEUS_LOOKAHEAD": "lookahead", "NEUS_EV_SYSFENCE": "ev_sysfence", "NEUS_LA_STAT": "la_stat",
    "NEUS_ADAM_OVERLAP": "adam_overlap", "NEUS_EXCHANGE_OVERLAP": "exchange_overlap", "NEUS_EAGER_EMA_H": "eager_ema_h",
    "NEUS_MARCH_BALANCE": "march_balance", "NEUS_RAY_CULL": "ray_cull", "NEUS_RAY_SORT": "ray_sort", "NEUS_PROG_CUT": "prog_cut",
    "NEUS_MARCH_CUT": "march_cut", "NEUS_OCC_SORT": "occ_sort", "NEUS_OCC_NU_SORT": "occ_nu_sort", "NEUS_SCATTER_NOSKIP": "scatter_noskip",
    "NEUS_DBG_LOSS_REPLAY": "dbg_loss_replay", "NEUS_DBG_LOSS_FENCE": "dbg_loss_fence", "NEUS_INFER_XCD_PARTS": "infer_xcd_parts",
    "NEUS_INFER_PIPE": "infer_pipe",
}


@pytest.mark.parametrize("var", sorted(SWITCHES))
def test_every_switch_has_its_own_variable(probe, var):
    """A switch flips with its own variable (default on: "0", default off: "1") and with no other."""
    f = SWITCHES[var]
    assert probe(**{var: "0" if DEFAULTS[f] == "1" else "1"}) == DEFAULTS | {f: "0" if DEFAULTS[f] == "1" else "1"}


@pytest.mark.parametrize("env,want", [
    ({"NEUS_MARCH_LANES": "1"}, {"march_lanes": "1"}),
    ({"NEUS_MARCH_LANES": "4"}, {"march_lanes": "4"}),
    ({"NEUS_MARCH_LANES": "8"}, {"march_lanes": "8"}),
    ({"NEUS_MARCH_LANES": "16"}, {"march_lanes": "16"}),
    ({"NEUS_MARCH_LANES": "3"}, {"march_lanes": "8"}),
    ({"NEUS_SCATTER_CHUNK": "1024"}, {"scatter_chunk": "1024"}),
    ({"NEUS_SCATTER_CHUNK": "256"}, {"scatter_chunk": "256"}),
    ({"NEUS_SCATTER_CHUNK": "2560"}, {"scatter_chunk": "512"}),
    ({"NEUS_SCATTER": "binned"}, {"scatter_mode": "1"}),
    ({"NEUS_SCATTER": "wide"}, {"scatter_mode": "0"}),
    ({"NEUS_SCATTER": "regions"}, {"scatter_mode": "2"}),
    ({"NEUS_SCATTER": "wide", "NEUS_SCATTER_CHUNK": "256"}, {"scatter_mode": "0", "scatter_chunk": "512"}),
    ({"NEUS_SCATTER": "binned", "NEUS_SCATTER_CHUNK": "1024"}, {"scatter_mode": "1", "scatter_chunk": "1024"}),
    ({"NEUS_SCATTER_LG": "3"}, {"scatter_level_groups": "3"}),
    ({"NEUS_SCATTER_LG": "-2"}, {"scatter_level_groups": "0"}),
    ({"NEUS_SC_XCD_GROUP": "8"}, {"scatter_xcd_group": "8"}),
    ({"NEUS_SC_XCD_GROUP": "0"}, {"scatter_xcd_group": "1"}),
    ({"NEUS_DBG_MARCH_CUT_DIV": "8"}, {"march_cut_div": "8"}),
    ({"NEUS_DBG_MARCH_CUT_DIV": "0"}, {"march_cut_div": "1"}),
    ({"NEUS_CHUNK_ENDS": "32,80"}, {"chunk_ends": "32,80"}),
    ({"NEUS_CHUNK_ENDS": "7"}, {"chunk_ends": "7"}),
    ({"NEUS_CHUNK_ENDS": ",".join(str(k) for k in range(1, 15))}, {"chunk_ends": ",".join(str(k) for k in range(1, 15))}),
    ({"NEUS_CHUNK_ENDS": "80,32"}, {}),
    ({"NEUS_CHUNK_ENDS": "32,32"}, {}),
    ({"NEUS_CHUNK_ENDS": "0,8"}, {}),
    ({"NEUS_CHUNK_ENDS": ""}, {}),
    ({"NEUS_CHUNK_ENDS": ",".join(str(k) for k in range(1, 16))}, {}),
    ({"NEUS_LA_PRIO": "1", "NEUS_LA_AT": "3", "NEUS_LA_AT_FULL": "2"}, {"la_prio": "1", "la_at_cut": "3", "la_at_full": "2"}),
    ({"NEUS_CHUNK_SCALE": "1.5", "NEUS_CHUNK_ROUNDS": "3"}, {"chunk_scale": "1.5", "chunk_rounds": "3"}),
    ({"NEUS_MLP_BLOCKS_PCT": "50", "NEUS_INFER_GRID": "64"}, {"mlp_blocks_pct": "50", "infer_grid": "64"}),
    ({"NEUS_INFER_XCD_PARTS": "1", "NEUS_INFER_PIPE": "0"}, {"infer_xcd_parts": "1", "infer_pipe": "0"}),
    ({"NEUS_MARCH_WAVES": "2048", "NEUS_MARCH_DBG": "2"}, {"march_waves": "2048", "march_dbg": "2"}),
    ({"NEUS_MAIN_PRIO": "0"}, {"main_prio": "0"}),
    ({"NEUS_MAIN_PRIO": "off"}, {}),
    ({"NEUS_DBG_POISON": "255"}, {"poison": "1", "byte": "255"}),
    ({"NEUS_DBG_POISON": "0:3:9"}, {"poison": "1", "byte": "0", "lo": "3", "hi": "9"}),
    ({"NEUS_DBG_POISON": "x"}, {}),
    ({"NEUS_DBG_ALLOC_LOG": "0"}, {"log": "1"}),
])
def test_special_forms(probe, env, want):
    """Each rule as the code had it before the table (not as its comments described it); every other field stays at
    its default."""
    assert probe(**env) == DEFAULTS | want
