"""The four two-launch BatchNorm training kernels on the BatchNorm shapes of the flagship generator (unconditional TGANv2,
B = 32: what tools/bn_bits.py records from one forward), REPS forward + adjoint pairs per shape through the C ABI with ReLU. Meant
to run under `rocprofv3 --kernel-trace --stats -- python tools/bn_passes_micro.py`, once per build of the library (T2V_LIB):
the kernel statistics then give each kernel's time over the same launches. Prints the wall time per pair as a cross-check."""
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from txt2vid_amd._lib import lib                    # noqa: E402
from txt2vid_amd._ops import _stream                # noqa: E402

SHAPES = [(512, 1024, 1), (512, 512, 4), (512, 256, 16), (512, 128, 64), (128, 128, 64), (128, 64, 256), (32, 64, 256), (32, 32, 1024),
          (8, 32, 1024), (8, 32, 4096)]
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DEV = 'cuda:0'


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    L, st = lib(), _stream()
    torch.manual_seed(3)
    for N, Cc, S in SHAPES:
        x, gy = torch.randn(N, Cc, S, device=DEV) + 1.0, torch.randn(N, Cc, S, device=DEV)
        gamma, beta, rm, rv = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        y, gx, stats = torch.empty_like(x), torch.empty_like(x), torch.empty(2 * Cc, device=DEV)
        dg, db = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
        ws = torch.empty(int(L.t2v_bn_ws_floats(N, Cc, S)), device=DEV)

        def pair():
            a = L.t2v_bn_train_fwd(p(x), p(gamma), p(beta), p(y), p(stats), p(rm), p(rv), p(ws), N, Cc, S, 0.1, 1e-5, 1, None, st)
            b = L.t2v_bn_train_bwd(p(gy), p(x), p(y), p(stats), p(gamma), p(gx), p(dg), p(db), p(ws), N, Cc, S, 1, st)
            assert a == 0 and b == 0, (a, b)
        for _ in range(5):
            pair()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            pair()
        torch.cuda.synchronize()
        print('bn-micro [%d,%d,%d] %.1f us per forward + adjoint pair' % (N, Cc, S, (time.perf_counter() - t0) / REPS * 1e6))


if __name__ == '__main__':
    main()
