#!/bin/bash
# Generate .mid files from the latent space of a model trained by scripts/train-vae.sh: every melody of the first batch in every
# class, from one encode. Other modes: --mode prior|posterior|interpolate|blend, and on an existing piece --mode continue --prime N
# [--n K] | repaint [--keep-time A B] [--keep-pitch LO HI] | score (python -m ...generate --help); whatever the caller
# passes in "$@" is appended (e.g. --mode interpolate --pair 0 3 --steps 9 --decoder greedy). The draw of --decoder sampling is the raw
# softmax as set below; flags in "$@" come later and win, e.g. scripts/generate-vae.sh --sample-temperature 0.9 --top-k 40 --top-p 0.9.
# --mode likelihood --iw-samples K prints the importance-weighted bound on log p(x) of every melody from K posterior draws (nll, elbo_nll,
# ess, bits per cell, valid), one line per melody, and writes no files.
# --ema (also through "$@") decodes with the checkpoint's averaged weights, for a model trained with --ema-decay.
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
--sample-temperature 1.0 \
--top-k 0 \
--top-p 1.0 \
--seed 0 \
--out /tmp/out/generated "$@"
