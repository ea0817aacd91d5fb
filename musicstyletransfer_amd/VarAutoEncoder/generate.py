"""Generation from the latent space under the reference's package layout:

    python -m music_style_transfer.VarAutoEncoder.generate --model-output DIR --mode transfer --data MIDI_DIR --out OUT_DIR

The implementation is musicstyletransfer_amd/generate.py."""
from ..generate import *  # noqa: F401,F403
from ..generate import build_parser, main  # noqa: F401

if __name__ == "__main__":
    main()
