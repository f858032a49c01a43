"""Learning-rate schedules of the retrieval model's training loop (reference train_decoder.py:151)."""
