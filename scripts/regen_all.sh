#!/bin/bash
# Regenerates every checked-in main-loop statement (constriction_amd/csrc/*.inc): the manifest is scripts/loops.py.
exec python "$(dirname "$0")/loops.py" "$@"
