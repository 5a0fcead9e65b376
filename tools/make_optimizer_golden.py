"""Record what a build of the library computes for the slot optimizers' dense, multi-tensor and row steps (the calls of
tests/optimizer_family_cases.py, through the C entry points alone), for tests/test_optimizer_family_golden_gpu.py to hold later
builds to:  python tools/make_optimizer_golden.py [--lib PATH] [--out tests/golden/optimizer_steps_parent.npz]
--lib: another build of libdt_hip.so with the same C ABI (the parent commit's, to record what a refactor must reproduce)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'optimizer_steps_parent.npz'))
    a = ap.parse_args()
    from deeptables_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from tests import optimizer_family_cases as C
    lib = _lib.lib()
    inputs_hash, out = C.run(lib)
    again = C.run(lib)[1]                      # the record must not depend on the run
    names = sorted(out)
    assert all(np.array_equal(C.digest(out[k]), C.digest(again[k])) for k in names), 'two runs of one build differ'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, inputs_hash=np.array(inputs_hash), source_hash=np.array(lib.dt_source_hash().decode()),
                        names=np.array(names), digests=np.stack([C.digest(out[k]) for k in names]))
    print(f'{a.out}: {len(names)} arrays, {sum(out[k].numel() * 4 for k in names)} bytes digested, {os.path.getsize(a.out)} '
          f'bytes written; library source hash {lib.dt_source_hash().decode()}, inputs {inputs_hash[:16]}')


if __name__ == '__main__':
    main()
