"""The wrapper modules behind vist3a_amd.ops, which re-exports them: import that, not these."""
