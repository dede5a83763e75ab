"""Writes tests/golden/key_runs_pins.npz on an MI355X: the outputs of gpsat_glue_keyed_batch and gpsat_glue_keyed_grad_batch on
the cases of tests/key_runs_cases.py, as the library of the checked-out commit returns them.  The keyed glues are held to
their restatements by a tolerance only (tests/test_gpu_cv_glue.py, tests/test_gpu_glue_grad.py); these pins hold the bytes,
so that a change to the sort-and-run-heads stage or to the walk of a group shows.  Run once at the commit whose bytes are to
be kept (here: the parent of the commit that gave the stage one implementation):

    python tests/golden/make_key_runs_pins.py [OUT.npz]

The file holds one array per field, the cases' records one behind the other in the order of key_runs_cases.CASES (key_runs_cases.unpack
takes them apart): crc (of a case's inputs) and G per case; out_key, out_count, out (the keyed glue of the value column) and
val_key, val_count, out_val, out_grad ([ndim, G], flattened) of the glue with gradient.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import key_runs_cases as kc  # noqa: E402


def main():
    from gpsat_amd.engine import default_engine
    eng = default_engine()
    pins = kc.pack([kc.outputs(eng, kind, R) for kind, R in kc.CASES])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "key_runs_pins.npz")
    np.savez_compressed(path, **pins)
    print(len(kc.CASES), "cases,", int(pins["G"].sum()), "groups,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
