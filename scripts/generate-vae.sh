#!/bin/bash
# Generate .mid files from the latent space of a model trained by scripts/train-vae.sh: every melody of the first batch in every
# class, from one encode. Other modes: --mode prior|posterior|interpolate|blend (python -m ...generate --help); whatever the caller
# passes in "$@" is appended (e.g. --mode interpolate --pair 0 3 --steps 9 --decoder greedy).
cd "$(dirname "$0")/.." || exit 1

python -m music_style_transfer.VarAutoEncoder.generate \
--model-output models/guitar_bass \
--checkpoint -1 \
--mode transfer \
--data "${MST_DATA:-./work/data/guitar_bass}" \
--max-seq-len 64 \
--slices-per-quarter-note 4 \
--batch-size 8 \
--temperature 1.0 \
--decoder sampling \
--seed 0 \
--out /tmp/out/generated "$@"
