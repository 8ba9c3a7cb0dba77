"""The module-scoped `mg` fixture of the GPU test files, once."""
import pytest


def gpu_module(**restore):
    """`mg = gpu_module(rb_exact=0)`: the package on cuda:0, quiet and with no grid; at the end of the file the grid is gone again and
    every option named here is back at the value given (options survive nhydro_clean, and the files that run later read them)."""
    @pytest.fixture(scope="module")
    def mg():
        import torch
        assert torch.cuda.is_available()
        torch.cuda.set_device(0)
        import mgroms_amd as m
        m.nhydro.set_verbose(0)
        m.nhydro_clean()
        yield m
        m.nhydro_clean()
        for name, value in restore.items():
            m.nhydro.set_option(name, value)
    return mg


def restore_options(*names):
    """`_restore_options = restore_options("krylov", ...)`: an autouse fixture that puts the named options back after every test of the file
    (the options a file touches survive nhydro_clean, and the tests that run after it read them)."""
    @pytest.fixture(autouse=True)
    def _restore_options(mg):
        keep = {k: mg.nhydro.get_option(k) for k in names}
        yield
        for k, v in keep.items():
            mg.nhydro.set_option(k, v)
    return _restore_options
