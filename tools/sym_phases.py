"""Where a k_symbols_reg wave spends its life, from a library built with -DDSA_SYM_STAMPS (make EXTRA=-DDSA_SYM_STAMPS; DSA_LIB
names it): python tools/sym_phases.py [meshes].  Per attribute of the bench mesh, median over sampled meshes, in M shader clocks:
set-up (tables, initial state), block loop, and what follows the loop up to early_tail (the slot -> symbol pass where there is one,
the drain of the last block where there is not).  A product library leaves these slots to other diagnostics: zeros."""
import sys, os; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, draco_sharp_amd as dsa, draco_sharp_amd.synth as synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
blob, offs = synth.make_batch(synth.GRID, 128, 256, 1000, n)
ctx = dsa.Context(0)
b = dsa.Batch(ctx, blob=blob, offsets=offs)
for _ in range(2): b.decode()
d = np.array([b.debug_array(i, 4, np.uint32, 20) for i in range(0, n, max(1, n // 64))])
h = np.ascontiguousarray(d).view(np.uint16).reshape(len(d), 40)
k = np.concatenate([h[:, 20:26], h[:, 36:39]], axis=1).astype(np.float64) * 1024 / 1e6      # half-word 3 p + ai
med = np.median(k, axis=0).reshape(3, 3)                                                      # [phase][attribute]
for ai in range(3):
    tot = med[:, ai].sum()
    print("attribute %d: set-up %.3f  loop %.3f  behind the loop %.3f  (M clocks; %.1f %% / %.1f %% / %.1f %% of %.3f)" %
          ((ai,) + tuple(med[:, ai]) + tuple(100 * med[:, ai] / max(tot, 1e-9)) + (tot,)))
