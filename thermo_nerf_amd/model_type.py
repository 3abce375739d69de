"""Which of the reference's four methods a command line names.  Names and integer values are the reference's own
[REF thermo_nerf/model_type.py:4-8]: they are what its command lines accept and what ``calculate_threshold`` switches on.  Only
THERMONERF is built here; the nerfacto-track and concat baselines are named so that a command line can refuse them by name."""
from enum import Enum

_VALUES = {"THERMALNERFACTO": 1, "THERMONERF": 2, "CONCATNERF": 3, "NERFACTO": 4}

ModelType = Enum("ModelType", _VALUES, module=__name__)
