"""Worker of test_options_surface_matches_record and test_option_environment_presets: what the library answers about its run-time options,
in a process of its own (the record changes options and calls mgx_clean; the environment presets act once, inside mgx_init).

  surface                  no GPU: for every option name, the answers of mgx_get_option, of mgx_set_option with a legal non-default value, of
                           mgx_get_option after it and after a following mgx_clean, then the texts of the errors; one JSON document on stdout
  env VARIABLE VALUE NAME  GPU: VARIABLE=VALUE in the environment, nhydro_init at 32x32x8, prints `VALUE <mgx_get_option(NAME)>`

tests/golden/options_surface.json is the output of both modes from the library as it was before the options were put into one table."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# every name either if/else chain of that library knew, without the three *_timeout_ms names (setting them writes a device constant);
# the value is the legal non-default value the record sets
NAMES = {
    "bmask": 1, "nsmall": 16, "solver_maxiter": 7, "ns_coarsest": 7, "ns_pre": 7, "ns_post": 7, "netcdf_output": 1, "aggressive": 1,
    "warm_start": 1, "tictoc": 1, "exact_halos": 1, "verbose": 0, "rb_chain": 0, "rb_exact": 1, "rb_seq": 0, "keep_r": 1, "c2f_skip": 0,
    "fuse_closing": 0, "restrict_chain": 0, "rbseq_fuse": 0, "rbseq_window": 0, "rbseq_rowcut": 0, "coarsest_direct": 2,
    "coarsest_direct_solves": 1, "rbseq_window_colours": 1, "rbseq_fuse_min": 12345, "rbseq_d0_in_pass": 0, "overlap": 1,
    "overlapped_passes": 1, "ksp": 0, "async": 1, "fuse_tail": 0, "cycle_precision": 32, "mixed_iterations": 1, "krylov": 3,
    "krylov_restarts": 1, "p2p_failed": 1, "p2p": 0, "ksp_test_stall": 1, "rbseq_test_stall": 1, "p2p_test_drop": 1,
}
ERRORS = [("set", "cycle_precision", 48), ("set", "krylov", 9), ("set", "krylov", -1), ("set", "p2p", 1), ("set", "bmask", 1),
          ("set", "coarsest_direct_solves", 1), ("set", "no_such_option", 1), ("get", "no_such_option", 0)]


def surface():
    from mgroms_amd._lib import lib
    L = lib()
    v = ctypes.c_int()

    def get(name):
        return v.value if L.mgx_get_option(name.encode(), ctypes.byref(v)) == 0 else None

    def err():
        return L.mgx_last_error().decode()

    rec = {"options": {}, "errors": []}
    for name, value in NAMES.items():
        r = {"default": get(name), "set_value": value}
        r["set_rc"] = L.mgx_set_option(name.encode(), value)
        r["set_error"] = err() if r["set_rc"] else None
        r["after_set"] = get(name)
        L.mgx_clean()
        r["after_clean"] = get(name)
        if r["set_rc"] == 0 and r["default"] is not None:
            assert L.mgx_set_option(name.encode(), r["default"]) == 0 and get(name) == r["default"], name
        elif r["set_rc"] == 0:   # the test hooks are write-only: off again
            assert L.mgx_set_option(name.encode(), 0) == 0, name
        rec["options"][name] = r
    for what, name, value in ERRORS:
        rc = L.mgx_set_option(name.encode(), value) if what == "set" else L.mgx_get_option(name.encode(), ctypes.byref(v))
        rec["errors"].append({"call": what, "name": name, "value": value, "rc": rc, "error": err() if rc else None})
    print(json.dumps(rec, indent=1))


def env(variable, value, name):
    os.environ[variable] = value
    import torch
    import mgroms_amd as mg
    from mgroms_amd import nhydro
    torch.cuda.set_device(0)
    nhydro.set_verbose(0)
    mg.nhydro_init(32, 32, 8, 1, 1, 0, nhydro.default_params())
    print("VALUE", nhydro.get_option(name))
    mg.nhydro_clean()


if __name__ == "__main__":
    if sys.argv[1] == "surface":
        surface()
    else:
        env(*sys.argv[2:5])
