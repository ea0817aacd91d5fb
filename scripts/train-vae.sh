#!/bin/bash
# Same invocation as the reference's scripts/train-vae.sh:5-29 (its venv line :3 is the only part that may
# differ per machine): the module path, every flag and every value are the reference's. Two flags are appended
# for this implementation: --gpu (the step has no CPU path) and, optionally, whatever the caller passes in "$@"
# (e.g. --pianoroll, --max-steps 200, --dtype fp16).
#   --d-input-dropout P   hide each decoder input position (the previous frame / token) with probability P in training steps, so the
#                         decoder has to use the latent (against posterior collapse, beside --kl-warmup-steps / --kl-free-bits); 0: off
#   --latent-stats        log per-dimension statistics of the posterior, summed on the device inside the step: active_units,
#                         kl_dims_used, kl_dim_max, sigma_rms and class_leak (how much of z's variation is between the classes)
#   --iw-samples K        after every checkpoint's validation pass, score the validation set with the importance-weighted bound on
#                         log p(x) from K posterior draws per piece: iw_nll, iw_elbo_nll, iw_gap, iw_ess, iw_bits_per_cell; 0: off
#   --class-mmd LAMBDA    add LAMBDA times the class-conditional MMD of z (each class's z against the pooled batch, RBF kernel) to the
#                         training objective, inside the step: the remedy when class_leak is near 1; class_mmd joins the log; 0: off
#                         (--class-mmd-bandwidth S2: the kernel's bandwidth, 0: the latent width)
cd "$(dirname "$0")/.." || exit 1

python -m music_style_transfer.VarAutoEncoder.main \
--batch-size 32 \
--kl-loss 1.0 \
--validation-split 0.0 \
--max-seq-len 64 \
--slices-per-quarter-note 4 \
--data "${MST_DATA:-./work/data/guitar_bass}" \
--model-output models/guitar_bass \
--out-samples /tmp/out \
--sampling-frequency 2000 \
--checkpoint-frequency 1000 \
--num-checkpoints-not-improved 32 \
--epochs 10000 \
--optimizer adam \
--optimizer-params clip_gradient:1.0 \
--learning-rate 0.0003 \
--label-smoothing 0.0 \
--e-n-layers 2 \
--e-dropout 0.2 \
--e-rnn-hidden-dim 256 \
--e-emb-hidden-dim 256 \
--latent-dim 256 \
--d-n-layers 1 \
--d-rnn-hidden-dim 128 \
--d-dropout 0.2 \
--gpu "$@"
