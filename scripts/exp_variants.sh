#!/bin/bash
# The serial form of this script wrote its experiment loops into the checked-in tree; there is one form now.
exec "$(dirname "$0")/exp_variants_par.sh" "$@"
