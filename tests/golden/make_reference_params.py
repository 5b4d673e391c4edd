"""Generator of tests/golden/reference_param_files.json: the parameter trees (yaml.safe_load) of the four parameter files the reference ships -- the car-like and the two
diff-drive example files of mpc_local_planner_examples/cfg/ and the test node's mpc_local_planner/cfg/test_mpc_optim_node.yaml.  Run where the reference tree exists:
    python tests/golden/make_reference_params.py REFERENCE_ROOT
tests/test_params.py::test_the_references_own_parameter_files_load reads these recorded trees, and compares them with the files themselves where the tree is present."""
import json
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FILES = ["mpc_local_planner_examples/cfg/carlike/mpc_local_planner_params.yaml",
         "mpc_local_planner_examples/cfg/diff_drive/mpc_local_planner_params_quadratic_form.yaml",
         "mpc_local_planner_examples/cfg/diff_drive/mpc_local_planner_params_minimum_time.yaml",
         "mpc_local_planner/cfg/test_mpc_optim_node.yaml"]
OUT = os.path.join(ROOT, "tests", "golden", "reference_param_files.json")


def load(ref_root):
    trees = {}
    for rel in FILES:
        with open(os.path.join(ref_root, rel)) as f:
            trees[rel] = yaml.safe_load(f) or {}
    return trees


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/golden/make_reference_params.py REFERENCE_ROOT")
    trees = load(sys.argv[1])
    assert json.loads(json.dumps(trees)) == trees, "a parameter tree does not survive JSON"
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_reference_params.py", "files": trees}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(OUT, ROOT), {k: len(v) for k, v in trees.items()})
