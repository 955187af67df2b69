"""Device-buffer plumbing for the GPU parity tests (torch only allocates and copies)."""
import contextlib
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_KEEP = []


def dev(t, a):
    """numpy -> torch cuda tensor with the same bytes. The tensor is kept alive until release()
    so that an inline `ptr(dev(...))` cannot hand a freed (and reused) block to a kernel."""
    x = _dev(t, a)
    _KEEP.append(x)
    return x


def release():
    _KEEP.clear()


def _dev(t, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float16 or a.dtype == np.uint16:
        return t.from_numpy(a.view(np.int16).copy()).cuda()
    if a.dtype == np.uint32:
        return t.from_numpy(a.view(np.int32).copy()).cuda()
    if a.dtype == np.uint8:
        return t.from_numpy(a.copy()).cuda()
    if a.dtype == np.uint64:
        return t.from_numpy(a.view(np.int64).copy()).cuda()
    return t.from_numpy(a.copy()).cuda()


def host(x, dtype):
    a = x.detach().cpu().numpy()
    return a.view(dtype)


def ptr(x):
    return C.c_void_p(x.data_ptr() if x is not None else 0)


@contextlib.contextmanager
def env(**kv):
    """The environment variables kv set (a None value: removed) inside the block, their previous values restored on every
    exit path. A testbed reads its NEUS_* switches when it is created: the block covers the creation, and by habit the
    dataset and the network load as well."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


OCC_BUFFERS = {"lin": (40, np.uint32, 128 ** 3 // 32), "bbox": (41, np.float32, 6), "mean": (42, np.float32, 1),
               "density_tmp": (43, np.float32, 128 ** 3)}


def occ_buffer(tb, name):
    """One product of the occupancy update / bitfield rebuild through neus_debug_get_buffer: "lin" (the march's words of
    the testbed's own field), "bbox", "mean" or "density_tmp"."""
    from neus2_amd._lib import check, lib
    bid, dtype, n = OCC_BUFFERS[name]
    a = np.zeros(n, dtype)
    check(lib().neus_debug_get_buffer(tb.handle, C.c_int(bid), C.c_uint64(0), C.c_uint64(a.nbytes), C.c_void_p(a.ctypes.data)))
    return a


def scatter_testbed(sc, mode, batch):
    """A base.json testbed on scene sc in one of the grid-gradient scatter modes: "regions" (per-block record regions,
    512-sample workgroups: the default), "regions1024" (1024-sample ones), "seg" (wide-block binning, 512), "seg1024" or
    "binned" (the 256-sample histogram / scan / bin path)."""
    from neus2_amd import pyngp
    with env(NEUS_SCATTER={"binned": "binned", "seg": "wide", "seg1024": "wide"}.get(mode),
             NEUS_SCATTER_CHUNK="1024" if mode.endswith("1024") else None):
        tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
        tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
        tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=batch)
    return tb
