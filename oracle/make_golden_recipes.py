#!/usr/bin/env python3
"""Generate tests/golden/gold_recipe_yaml.json: the values of the reference's shipped recipe YAMLs that
articulatory_amd/utils/recipes.py restates (tests/test_train_host.py::test_recipe_values_equal_the_shipped_yaml).

Run where the reference repository is checked out, with HIFICAR_REFERENCE naming that checkout:

    HIFICAR_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_recipes.py

Only data is written: for each YAML, the parsed value of every top-level key the restatement carries
(the keys the test compares) and `discriminator_params`, keyed by the YAML's path inside the reference.
"""

import json
import os
import sys

import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ["HIFICAR_REFERENCE"]
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

RECIPES = {"car": "egs/ema/voc1/conf/e2w_hifigan_car.yaml", "e2w": "egs/ema/voc1/conf/e2w_hifigan.yaml",
           "mri": "egs/mri/voc1/conf/mri2w_hifigan_car.yaml"}
NOT_COMPARED = ("distributed", "fused_optimizers", "stft_loss_params")


def main():
    from articulatory_amd.utils.recipes import recipe_train_config

    out = {}
    for recipe, path in RECIPES.items():
        with open(os.path.join(REF, path)) as f:
            ref = yaml.safe_load(f)
        keys = [k for k in recipe_train_config(recipe) if k not in NOT_COMPARED and k in ref] + ["discriminator_params"]
        out[path] = {k: ref[k] for k in keys}
    dst = os.path.join(REPO, "tests", "golden", "gold_recipe_yaml.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
