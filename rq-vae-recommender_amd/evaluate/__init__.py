"""Evaluation metrics — drop-in for the reference's evaluate package."""
